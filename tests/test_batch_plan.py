"""CPU-only: how a batch is cut into work units and which kernel it is dispatched to (xgm_batch_plan.cc::xgm_plan_batch),
on a host-only index — also with probe containers and flat posting arrays pretended (xgm_debug_set_plan_facts), so that the
bodies of the conjunction kernel, xgm_orw2_kernel, the LIST and the COUNT launches are planned here.  Invariants: the units of every query tile its stripes exactly once, every unit's output
slot is unique and inside the query's slot range, the per-query unit count fits the merge kernel; dispatch: a batch
goes to the wave-autonomous kernels only when every query of it has the shape they implement."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import helpers as H
from xapiand_amd import Database, Query, _lib
from xapiand_amd.enquire import plan


@pytest.fixture(scope="module")
def facts_seg(built, tmp_path_factory):
    return H.Corpus(120000, 200000).build_segment(str(tmp_path_factory.mktemp("bp") / "c.seg"))      # 15 stripes of 8192 docids


@pytest.fixture(scope="module")
def host_db(facts_seg):
    db = Database(facts_seg, device=_lib.XGM_DEVICE_NONE)
    yield db
    db.close()


def plan_batch(db, queries, first=0, maxitems=10):
    L = _lib.lib()
    L.xgm_debug_plan_batch.restype = C.c_int64
    L.xgm_debug_plan_batch.argtypes = [C.c_void_p, C.POINTER(_lib.Query), C.c_uint32, C.c_char_p, C.POINTER(C.c_uint32), C.c_uint64]
    plans = [plan(db, q, first, maxitems) for q in queries]
    arr = (_lib.Query * len(plans))(*plans)
    name = C.create_string_buffer(32)
    cap = 1 << 16
    units = (C.c_uint32 * (4 * cap))()
    n = L.xgm_debug_plan_batch(db._h, arr, len(plans), name, units, cap)
    if n > 0 and n > cap:
        raise AssertionError("too many units")
    _lib.check(min(0, n) if n < 0 else 0)
    if n == _lib.XGM_UNSUPPORTED:
        raise _lib.XgmUnsupported()
    return name.value.decode(), [tuple(units[4 * i:4 * i + 4]) for i in range(n)]


def term_queries(op, n, nt, seed, **kw):
    return [Query(q["op"], q["terms"], n_required=q.get("n_required", 0)) for q in H.gen_term_queries(op, n, nt, 1, 4096, seed=seed, **kw)]


def sided_queries(op, n, nr, no, seed):
    return [Query(q["op"], q["terms"], n_required=q["n_required"]) for q in H.gen_sided_queries(op, n, nr, no, 1, 500, 1, 4096, seed=seed)]


def check_units(db, nq, units):
    n_stripes = (db.info().lastdocid >> 13) + 1
    per = {}
    for qi, sb, se, slot in units:
        assert qi < nq and sb < se <= n_stripes
        per.setdefault(qi, []).append((sb, se, slot))
    assert sorted(per) == list(range(nq))
    slots = sorted(s for u in per.values() for _, _, s in u)
    assert slots == list(range(len(units)))                       # dense, unique output slots
    for qi, us in per.items():
        us.sort()
        assert us[0][0] == 0 and us[-1][1] == n_stripes
        assert all(a[1] == b[0] for a, b in zip(us, us[1:]))       # tiles the stripes exactly once
        s = sorted(x[2] for x in us)
        assert s == list(range(s[0], s[0] + len(us)))              # one contiguous slot range per query
        assert len(us) * 16 <= 8192


def test_units_tile_every_query(host_db):
    for queries, k in ((term_queries("AND", 40, 3, 1), 10), (term_queries("OR", 30, 5, 2), 100), (term_queries("AND", 3, 2, 3), 10)):
        name, units = plan_batch(host_db, queries, 0, k)
        check_units(host_db, len(queries), units)


def test_kernel_dispatch(host_db):
    AND, OR = term_queries("AND", 6, 3, 11), term_queries("OR", 6, 4, 12)
    assert plan_batch(host_db, AND)[0] == "xgm_andw_kernel"
    assert plan_batch(host_db, OR, 0, 100)[0] == "xgm_orw_kernel"
    assert plan_batch(host_db, AND + OR)[0] == "xgm_match_kernel"                         # ONE launch for mixed shapes: the general kernel
    assert plan_batch(host_db, AND, 0, 500)[0] == "xgm_and_kernel"                        # k beyond the wave kernel's buffer
    assert plan_batch(host_db, term_queries("AND", 2, 1, 13))[0] == "xgm_match_kernel"    # single-term queries
    phrase = [Query("PHRASE", q["terms"]) for q in H.gen_phrase_queries(4, 120000, 200000, seed=14)]
    assert plan_batch(host_db, phrase)[0] == "xgm_andw_kernel:phrase"
    assert plan_batch(host_db, phrase + AND)[0] == "xgm_andw_kernel:phrase"               # plain conjunctions ride along
    assert plan_batch(host_db, sided_queries("AND_NOT", 4, 2, 2, 15) + AND)[0] == "xgm_andw_kernel:sided1"
    assert plan_batch(host_db, sided_queries("AND_MAYBE", 4, 2, 2, 16) + sided_queries("AND_NOT", 2, 1, 1, 17))[0] == "xgm_andw_kernel:sided2"
    assert plan_batch(host_db, sided_queries("FILTER", 4, 2, 1, 18))[0] == "xgm_andw_kernel"   # a FILTER is a conjunction
    assert plan_batch(host_db, sided_queries("AND_MAYBE", 2, 3, 6, 19))[0] == "xgm_match_kernel"  # 9 terms: beyond the register program
    assert plan_batch(host_db, sided_queries("AND_NOT", 2, 2, 1, 20) + OR)[0] == "xgm_match_kernel"


def launches(db, queries, first=0, maxitems=10):
    plans = [plan(db, q, first, maxitems) for q in queries]
    arr = (_lib.Query * len(plans))(*plans)
    out = C.create_string_buffer(512)
    n = _lib.lib().xgm_debug_batch_launches(db._h, arr, len(plans), out, 512)
    assert n >= 0
    return out.value.decode().split(";")


def test_heterogeneous_batch_is_cut_by_kernel_class(host_db):
    """A server's natural batch mixes shapes: xgm_search_batch launches one kernel per class present instead of sending
    everything to the general workgroup kernel."""
    AND, OR = term_queries("AND", 6, 3, 11), term_queries("OR", 5, 4, 12)
    phrase = [Query("PHRASE", q["terms"]) for q in H.gen_phrase_queries(4, 120000, 200000, seed=14)]
    an, am = sided_queries("AND_NOT", 3, 2, 2, 15), sided_queries("AND_MAYBE", 2, 2, 2, 16)
    single = term_queries("AND", 2, 1, 13)
    assert launches(host_db, AND) == ["xgm_andw_kernel*6"]
    mixed = [AND[0], OR[0], phrase[0], an[0], AND[1], am[0], OR[1], single[0]] + AND[2:] + OR[2:] + phrase[1:] + an[1:] + am[1:] + single[1:]
    assert launches(host_db, mixed) == ["xgm_andw_kernel*6", "xgm_andw_kernel:sided1*3", "xgm_andw_kernel:sided2*2", "xgm_andw_kernel:phrase*4",
                                        "xgm_orw_kernel*5", "xgm_match_kernel*2"]
    big = sided_queries("AND_MAYBE", 2, 3, 6, 19)                   # 9 terms: beyond the register program → the general kernel
    assert launches(host_db, AND + big) == ["xgm_andw_kernel*6", "xgm_match_kernel*2"]
    # deep pages (first + maxitems > 192) leave the wave kernels without taking the shallow ones along
    plans = [plan(host_db, q, 0, 10) for q in AND[:4]] + [plan(host_db, q, 0, 500) for q in AND[4:]]
    arr = (_lib.Query * len(plans))(*plans)
    out = C.create_string_buffer(512)
    assert _lib.lib().xgm_debug_batch_launches(host_db._h, arr, len(plans), out, 512) == 2
    assert out.value.decode().split(";") == ["xgm_andw_kernel*4", "xgm_and_kernel*2"]


# ---- with acceleration structures pretended on a host-only index (XgmPlanFacts) ----------------------------------------------------

QF_DENSE, QF_FLAT = 64, 128           # xgm_device.h
DENSE_MIN_DF = 32 * 15                # xgm_build_dense's own threshold for this shard: XGM_DENSE_MIN_AVG postings per stripe


def open_with_facts(seg):
    db = Database(seg, device=_lib.XGM_DEVICE_NONE)
    _lib.check(_lib.lib().xgm_debug_set_plan_facts(db._h, DENSE_MIN_DF, 1 | 2 | 4 | 8, db.info().n_postings))
    return db


@pytest.fixture(scope="module")
def facts_db(facts_seg):
    db = open_with_facts(facts_seg)
    yield db
    db.close()


def plan_dump(db, queries, mode=0, force_general=0, maxitems=10):
    """(scalars by name, flags per query, units) of xgm_debug_plan_dump."""
    plans = [plan(db, q, 0, maxitems) for q in queries]
    arr = (_lib.Query * len(plans))(*plans)
    cap = 26 + len(plans) + 4 * (1 << 16)
    out = (C.c_uint64 * cap)()
    n = _lib.lib().xgm_debug_plan_dump(db._h, arr, len(plans), mode, force_general, out, cap)
    assert 26 <= n <= cap
    assert C.c_int64(out[0]).value == 0
    names = ("nq k_max tab_terms n_work stripes_per_group cap k_stride_c merge_cap phrase wide and_only andw sided orw fused parts sub_bits "
             "orw_planes orw2 or_flat").split()
    sc = dict(zip(names, out[1:21]))
    assert n == 26 + sc["nq"] + 4 * sc["n_work"]
    flags = list(out[26:26 + sc["nq"]])
    at = 26 + sc["nq"]
    return sc, flags, [tuple(out[at + 4 * i:at + 4 * i + 4]) for i in range(sc["n_work"])]


def rank_queries(op, groups):
    return [Query(op, ["t%d" % r for r in g]) for g in groups]


def test_frequent_conjunctions_take_the_dense_body(facts_db):
    qs = rank_queries("AND", [(1 + i, 8 + i, 20 + i) for i in range(6)])
    name, units = plan_batch(facts_db, qs)
    assert name == "xgm_andw_kernel"
    check_units(facts_db, len(qs), units)
    sc, flags, dunits = plan_dump(facts_db, qs)
    assert dunits == units and sc["andw"] == 1 and sc["fused"] == 1 and sc["parts"] == 1
    assert all(f & QF_DENSE and not f & QF_FLAT for f in flags)


def test_conjunction_led_by_a_rare_term_takes_the_flat_body(facts_db):
    qs = rank_queries("AND", [(3000 + i, 1 + i, 9 + i) for i in range(6)])
    name, units = plan_batch(facts_db, qs)
    assert name == "xgm_andw_kernel"
    check_units(facts_db, len(qs), units)
    _, flags, _ = plan_dump(facts_db, qs)
    assert all(f & QF_FLAT and not f & QF_DENSE for f in flags)


def orw2_child(seg):
    """(the body of test_short_disjunctions_go_to_orw2, in a process that has XGM_ORW2=1)"""
    db = open_with_facts(seg)
    # every term with a container -> 1; one long-tail term with a flat array per query -> 2
    for nt, tail, want in ((2, 0, 1), (5, 0, 1), (8, 0, 1), (7, 1, 2)):
        qs = rank_queries("OR", [tuple(1 + i + 7 * t for t in range(nt)) + ((4000 + i,) if tail else ()) for i in range(6)])
        name, units = plan_batch(db, qs, 0, 100)
        assert name == "xgm_orw2_kernel", name
        check_units(db, len(qs), units)
        assert plan_dump(db, qs, maxitems=100)[0]["orw2"] == want
    db.close()
    print("orw2 ok")


def test_short_disjunctions_go_to_orw2(facts_seg):
    """xgm_orw2_kernel is opt-in: XGM_ORW2=1, which the launch code reads once per process — hence the child process."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); import test_batch_plan as T; T.orw2_child(sys.argv[1])" % here, facts_seg],
                       env=dict(os.environ, XGM_ORW2="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "orw2 ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_list_plan_of_positional_queries(facts_db):
    """mode 1, xgm_andw_list_kernel's launch: one part, the units in stripe order.  (Terms of middling frequency: a few hundred documents of the
    conjunction per stripe, so that no unit is a part of a stripe and check_units' tiling applies as it stands.)"""
    qs = rank_queries("PHRASE", [(30 + i, 60 + i) for i in range(6)]) + rank_queries("PHRASE", [(40, 50, 70)])
    sc, flags, units = plan_dump(facts_db, qs, mode=1)
    assert sc["parts"] == 1 and sc["fused"] == 0 and sc["phrase"] == 1 and sc["andw"] == 1
    assert all(f & QF_DENSE for f in flags)
    assert all(se >> 24 == 0 for _, _, se, _ in units)
    assert [u[1] for u in units] == sorted(u[1] for u in units)          # launch order = stripe order
    assert len(units) > len(qs)
    check_units(facts_db, len(qs), units)


def test_count_plan_has_one_part(facts_db):
    qs = rank_queries("AND", [(1 + i, 8 + i, 20 + i) for i in range(6)]) + rank_queries("AND", [(3000, 1, 9)])
    sc, flags, units = plan_dump(facts_db, qs, mode=2)
    assert sc["parts"] == 1 and sc["fused"] == 0 and sc["andw"] == 1
    check_units(facts_db, len(qs), units)


@pytest.mark.gpu
def test_plan_facts_of_a_device_index_are_its_own(built, tmp_path):
    c = H.Corpus(20000, 50000)
    db = Database(c.build_segment(str(tmp_path / "d.seg")), device=0)
    try:
        assert _lib.lib().xgm_debug_set_plan_facts(db._h, 1, 3, 0) == -1       # XGM_E_INVALID
    finally:
        db.close()
