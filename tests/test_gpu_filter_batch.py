"""Several query filters in one launch, under a base filter (include/xgm.h: xgm_filter_build_query_batch): every bitmap of
xgm_filter_mark_query_batch_kernel word for word against Python set algebra over postings the test writes itself AND against the single-plan call
(xgm_filter_build_query, then xgm_filter_combine with the base filter) — at a word, a tile and one, two and three units of the kernel, with the 25
plans of tests/test_gpu_filter_query.py in ONE call —, the units skipped under a base filter, the batch sizes 1 .. XGM_FILTER_BATCH_MAX, the
grid-stride loop's later trips (XGM_FILTER_BATCH_MAX_GRID), the three membership sources, the independent device path (xgm_search_all), the shared
allocation's lifetime under every free order and from eight threads, and the all-or-nothing error table.

The same file runs under the CPU emulation of the kernels with guard pages behind every device buffer (tests/test_emu_filter_batch.py)."""
import collections
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import helpers as H
import test_gpu_filtered as F
from test_gpu_filter_query import FLAT_PLANS, SWITCHES, TREES, bools_of, eval_flat, eval_tree, manual_sets
from xapiand_amd import Database, Query, _lib
from xapiand_amd.enquire import count_pairs, filter_all, filter_and, plan, search_all, search_range

pytestmark = [pytest.mark.gpu]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = F.QUICK
INVALID, UNSUPPORTED, NO_DEVICE = _lib.XGM_E_INVALID, _lib.XGM_UNSUPPORTED, _lib.XGM_E_NO_DEVICE
BATCH_MAX = _lib.XGM_FILTER_BATCH_MAX
LASTDOCIDS = [1, 33, 2049, 8193, 16390]          # a word, a tile, and one, two and three units (the last of 6 documents)
STRIPE_BITS = [0, 8]
N_PLANS = len(FLAT_PLANS) + len(TREES)
P32 = C.POINTER(C.c_uint32)
UNIT_DOCS = 8192


def grid_cap():
    """The most workgroups the library launches the batch kernel with: XGM_FILTER_BATCH_MAX_GRID as the library reads it, else 8192."""
    try:
        v = int(os.environ.get("XGM_FILTER_BATCH_MAX_GRID", "0"))
    except ValueError:
        v = 0
    return v if 1 <= v <= 8192 else 8192


def n_units_of(lastdocid):
    n_padded = -(-((lastdocid + 32) // 32) // 64) * 64
    return -(-n_padded // 256)


def batch_info():
    out = (C.c_uint64 * 4)()
    assert _lib.lib().xgm_debug_filter_batch_info(out) == 0
    return list(out)           # kernel launches, (plan, unit) work items, waves launched, work items skipped under the base filter


def words(f):
    return np.array(f.words(), dtype=np.uint32)


class Shard:
    """manual_sets' postings and two more terms — `first`: documents of the first unit only, `last`: of the last unit only — as a segment, with the 25
    plans of tests/test_gpu_filter_query.py and what each matches by set algebra."""

    def __init__(self, tmp_path, lastdocid, stripe_bits, wdf255=False):
        self.last, n = lastdocid, lastdocid + 1
        self.sets, post = manual_sets(lastdocid, stripe_bits, wdf255)
        last_unit = (lastdocid // UNIT_DOCS) * UNIT_DOCS
        extra = {"first": sorted({1, min(lastdocid, 77), min(lastdocid, UNIT_DOCS - 1)}), "last": sorted({max(1, last_unit), lastdocid})}
        for k, docs in extra.items():
            self.sets[k] = np.zeros(n, dtype=bool)
            self.sets[k][docs] = True
            post[k] = [(d, 1) for d in docs]
        self.c = H.ManualCorpus(post, {d: 600 + d % 7 for d in range(1, n)}, positions=False)
        self.db = Database(self.c.build_segment(str(tmp_path / "b.seg"), stripe_bits=stripe_bits))
        assert self.db.get_lastdocid() == lastdocid
        self.plans, self.want = [], []
        for q in FLAT_PLANS:
            query = Query(q["terms"][0]) if len(q["terms"]) == 1 else Query(q["op"], q["terms"], n_required=q.get("n_required", 0))
            self.plans.append(plan(self.db, query, 0, 10))
            self.want.append(eval_flat(q, self.sets, n))
        for tree in TREES:
            self.plans.append(plan(self.db, Query.tree(tree), 0, 10))
            self.want.append(eval_tree(tree, self.sets, n))
        assert len(self.plans) == N_PLANS == 25 and sum(int(w.sum()) for w in self.want) > 0

    def term_filter(self, term):
        return self.db.build_query_filter(plan(self.db, Query(term), 0, 10))

    def singles(self):
        return [self.db.build_query_filter(p) for p in self.plans]

    def close(self):
        self.db.close()
        self.c.close()


def check_batch(s, under=None, under_set=None, singles=None):
    """One call over the 25 plans: every bitmap equals the set algebra (ANDed with under_set), the single-plan call's words (combined with `under`),
    and its count the popcount.  Returns the debug figures."""
    own = singles is None
    singles = s.singles() if own else singles
    got = s.db.build_query_filters(s.plans, under)
    info = batch_info()
    assert len(got) == N_PLANS
    for i, (g, one) in enumerate(zip(got, singles)):
        want = s.want[i] & under_set if under is not None else s.want[i]
        assert (bools_of(g, s.last) == want).all(), (s.last, i, np.nonzero(bools_of(g, s.last) != want)[0][:8])      # (bools_of: n_docs == the popcount)
        if under is None:
            assert g.words() == one.words() and g.n_docs == one.n_docs, (s.last, i)
        else:
            assert (words(g) == (words(one) & words(under))).all(), (s.last, i)
            both = filter_and(s.db, one, under)
            assert g.words() == both.words() and g.n_docs == both.n_docs, (s.last, i)
            both.close()
    n_items = n_units_of(s.last) * N_PLANS
    n_waves = min(n_items, grid_cap())
    n_waves -= n_waves % N_PLANS if n_waves > N_PLANS else 0             # a multiple of the plans where there are more waves than plans
    assert info[:3] == [1, n_items, n_waves], info
    for f in got + (singles if own else []):
        f.close()
    return info


# ---- 1. word for word ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stripe_bits", STRIPE_BITS)
@pytest.mark.parametrize("lastdocid", LASTDOCIDS)
def test_batch_word_for_word(built, tmp_path, lastdocid, stripe_bits):
    s = Shard(tmp_path, lastdocid, stripe_bits)
    info = check_batch(s)
    assert info[3] == 0                                                  # no base filter: nothing skipped
    s.close()


# ---- 2. under a base filter -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stripe_bits", STRIPE_BITS)
@pytest.mark.parametrize("lastdocid", [8193, 16390])
def test_batch_under_a_base_filter(built, tmp_path, lastdocid, stripe_bits):
    s = Shard(tmp_path, lastdocid, stripe_bits)
    singles = s.singles()
    n_units = n_units_of(lastdocid)
    live = np.ones(lastdocid + 1, dtype=bool)
    live[0] = False
    cases = [("bool", s.term_filter("bool"), s.sets["bool"], 0),                                       # set bits in every unit
             ("empty", s.term_filter("absent"), np.zeros(lastdocid + 1, dtype=bool), n_units * N_PLANS),
             ("all", filter_all(s.db), live, 0),
             ("first", s.term_filter("first"), s.sets["first"], (n_units - 1) * N_PLANS),              # documents of the first unit only
             ("last", s.term_filter("last"), s.sets["last"], (n_units - 1) * N_PLANS)]                 # ... of the last unit only
    for name, under, under_set, skipped in cases:
        assert (bools_of(under, lastdocid) == under_set).all(), name
        before = under.words()
        info = check_batch(s, under, under_set, singles)
        assert info[3] == skipped, (name, info)
        assert under.words() == before, name                             # the base filter is only read
        under.close()
    for f in singles:
        f.close()
    s.close()


# ---- 3. batch sizes -----------------------------------------------------------------------------------------------------------------------------------

def test_batch_sizes(built, tmp_path):
    s = Shard(tmp_path, 2049, 0)
    singles = s.singles()
    for n in (1, 2, BATCH_MAX):
        idx = [i % N_PLANS for i in range(n)]                            # the 25 plans repeated up to 64
        got = s.db.build_query_filters([s.plans[i] for i in idx])
        assert batch_info()[:2] == [1, n_units_of(2049) * n]
        all_words = [g.words() for g in got]
        for j, i in enumerate(idx):
            assert all_words[j] == singles[i].words() and got[j].n_docs == singles[i].n_docs, (n, j)
            assert all_words[j] == all_words[i], (n, j)                  # a duplicate gives identical words
        for g in got:
            g.close()
    l = _lib.lib()
    arr = (_lib.Query * (BATCH_MAX + 1))(*[s.plans[i % N_PLANS] for i in range(BATCH_MAX + 1)])
    hs = (C.c_void_p * (BATCH_MAX + 1))()
    for n in (BATCH_MAX + 1, 0):
        assert l.xgm_filter_build_query_batch(s.db._h, arr, n, None, hs, None) == INVALID and not any(hs)
    got = s.db.build_query_filters(s.plans[:3])                          # ... and a good call follows
    assert [g.words() for g in got] == [f.words() for f in singles[:3]]
    for f in got + singles:
        f.close()
    s.close()


# ---- 4. the stride loop; 5. the other sources: child processes (the switches are read once per process) ------------------------------------------

_first_failure = []


def run_child(env_add, select, n_passed):
    assert not _first_failure, "not run: %s" % _first_failure[0]          # one child after the other; after the first that fails none is started
    env = dict(os.environ, **env_add)
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", "-k", select],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        _first_failure.append("%s: killed at its time limit:\n%s" % (env_add, (e.stdout or b"")[-2000:]))
        raise AssertionError(_first_failure[0])
    if r.returncode != 0 or "%d passed" % n_passed not in r.stdout:
        _first_failure.append("%s failed with %d:\n%s\n%s" % (env_add, r.returncode, r.stdout[-3000:], r.stderr[-2000:]))
    assert not _first_failure, _first_failure[0]


@pytest.mark.parametrize("cap", [1, 2])
def test_batch_stride_loop(built, cap):
    """One and two workgroups for 75 work items: every trip of the grid-stride loop but the first, with and without a base filter, at three units."""
    run_child({"XGM_FILTER_BATCH_MAX_GRID": str(cap)}, "(test_batch_word_for_word or test_batch_under_a_base_filter) and 16390-0", 2)


@pytest.mark.parametrize("lastdocid", [8193] if QUICK else [33, 8193])
def test_batch_from_blocks_in_the_default_configuration(built, tmp_path, lastdocid):
    """A term whose wdf bound exceeds 254 has neither containers nor a flat array (tests/test_gpu_filter_query.py): the batch reads its BLOCKS."""
    s = Shard(tmp_path, lastdocid, 0, wdf255=True)
    check_batch(s)
    under = s.term_filter("third")
    check_batch(s, under, s.sets["third"])
    under.close()
    s.close()


@pytest.mark.parametrize("switch", SWITCHES)
def test_batch_with_a_source_switched_off(built, switch):
    if QUICK:
        pytest.skip("one emulated process per switch is not a quick run")
    run_child({k: "1" for k in switch.split()}, "(test_batch_word_for_word or test_batch_under_a_base_filter) and 8193-8", 2)


# ---- 6. against the independent device path -------------------------------------------------------------------------------------------------------------

def test_batch_equals_the_documents_search_all_lists(built, tmp_path):
    """The Zipf corpus of tests/test_gpu_filter_query.py's test 3, its queries sent in batches of 16: the docids xgm_search_all lists, the same count."""
    c = H.Corpus(*((2500, 6000) if QUICK else (4000, 10000)))
    db = Database(c.build_segment(str(tmp_path / "a.seg"), stripe_bits=10))
    last = c.v.lastdocid
    n = (lambda full, quick: quick if QUICK else full)
    queries = (H.gen_tree_queries(n(24, 12), 1, 600, seed=91) + H.gen_term_queries("AND", n(4, 2), 2, 1, 60, seed=92) + H.gen_term_queries("AND", n(3, 1), 3, 1, 40, seed=93) +
               H.gen_term_queries("OR", n(3, 1), 2, 1, 2000, seed=94) + H.gen_term_queries("OR", n(3, 1), 5, 1, 3000, seed=95) +
               H.gen_sided_queries("AND_NOT", n(4, 2), 1, 2, 1, 40, 1, 300, seed=96) + H.gen_sided_queries("AND_MAYBE", n(4, 2), 2, 2, 1, 40, 1, 300, seed=97) +
               H.gen_sided_queries("FILTER", n(4, 2), 1, 1, 1, 60, 1, 60, seed=98))
    plans = [plan(db, Query.tree(q["tree"]) if "tree" in q else Query(q["op"], q["terms"], n_required=q.get("n_required", 0)), 0, 10) for q in queries]
    n_some = 0
    for at in range(0, len(plans), 16):
        got = db.build_query_filters(plans[at:at + 16])
        for p, q, flt in zip(plans[at:], queries[at:], got):
            rows, hdr = search_all(db, p)
            assert np.nonzero(bools_of(flt, last))[0].tolist() == [d for d, _, _ in rows], q
            assert flt.n_docs == len(rows) == hdr.matches_exact, q
            n_some += 0 < len(rows) < last
            flt.close()
    assert n_some >= len(queries) // 2
    db.close()
    c.close()


# ---- 7. lifetime of the shared allocation ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["reverse", "interleaved"])
def test_batch_filters_freed_in_any_order(built, tmp_path, order):
    """All filters of a batch but one are freed — from the back, or odd ones first and then the even ones; the consumers over the survivor answer as over
    a filter built alone; then the survivor goes too."""
    last = 16390
    s = Shard(tmp_path, last, 0)
    rng = np.random.RandomState(7)
    ords = {}
    for slot, nd in ((0, 12), (1, 5)):
        o = rng.randint(0, nd + 1, size=last + 1).astype(np.uint32)
        o[0] = 0
        ords[slot] = o
        _lib.check(_lib.lib().xgm_index_attach_column_ordinals(s.db._h, slot, o.ctypes.data_as(P32), last + 1, nd))
    under = s.term_filter("bool")
    got = s.db.build_query_filters(s.plans, under)
    keep = 5 if order == "reverse" else 24                               # (the OR of two terms; the last plan of the batch: the last bitmap of the allocation)
    seq = list(range(N_PLANS - 1, -1, -1)) if order == "reverse" else list(range(1, N_PLANS, 2)) + list(range(0, N_PLANS, 2))
    for i in seq:
        if i != keep:
            got[i].close()
    one = s.db.build_query_filter(s.plans[keep])
    alone = filter_and(s.db, one, under)
    ok = s.want[keep] & s.sets["bool"]
    assert (bools_of(got[keep], last) == ok).all() and got[keep].n_docs == alone.n_docs > 0
    page = search_range(s.db, got[keep], 50)
    assert [d for d, _, _, _ in page[0]] == [int(d) for d in np.nonzero(ok)[0][:50]]
    assert page[0] == search_range(s.db, alone, 50)[0] and page[1].matches_exact == alone.n_docs
    cnt = collections.Counter((int(ords[0][d]), int(ords[1][d])) for d in np.nonzero(ok)[0])
    assert count_pairs(s.db, got[keep], 0, 1) == count_pairs(s.db, alone, 0, 1) == sorted((a, b, n) for (a, b), n in cnt.items())
    for f in (got[keep], one, alone, under):
        f.close()
    again = s.db.build_query_filters(s.plans[:2])                        # the index goes on building batches
    assert (bools_of(again[0], last) == s.want[0]).all() and (bools_of(again[1], last) == s.want[1]).all()
    again[1].close()
    again[0].close()
    s.close()


def test_batch_from_eight_threads_under_one_base_filter(built, tmp_path):
    last = 8193
    s = Shard(tmp_path, last, 0)
    under = s.term_filter("third")
    idx = [0, 3, 5, 6, 9, 16, 21, 24]
    plans = [s.plans[i] for i in idx]
    want = [(F_words(s.want[i] & s.sets["third"]), int((s.want[i] & s.sets["third"]).sum())) for i in idx]
    got, errors = {}, []
    gate = threading.Barrier(8)

    def work(t):
        try:
            gate.wait()
            out = []
            for _ in range(2):
                fs = s.db.build_query_filters(plans, under)
                out.append([(f.words(), f.n_docs) for f in fs])
                for f in (fs[t:] + fs[:t]):                              # every thread frees in an order of its own
                    f.close()
            got[t] = out
        except Exception as e:                                           # (an assertion inside a thread would be lost)
            errors.append(repr(e))
    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert len(got) == 8 and all(rep == want for t in range(8) for rep in got[t])
    under.close()
    s.close()


def F_words(ok):
    """One bool per docid 0 .. lastdocid → the words of xgm_filter_read, as a list."""
    padded = np.zeros((len(ok) + 31) // 32 * 32, dtype=np.uint8)
    padded[:len(ok)] = ok
    return np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32).tolist()


# ---- 8. all or nothing; the error table -------------------------------------------------------------------------------------------------------------------

def test_batch_all_or_nothing_and_errors(built, tmp_path):
    post = {"a": [(1, 1, [1]), (2, 1, [1]), (40, 2, [3, 9])], "b": [(1, 1, [2]), (2, 1, [7]), (50, 1, [1])], "c": [(2, 1, [3]), (40, 1, [4])]}
    c = H.ManualCorpus(post, {d: 10 for d in range(1, 51)}, positions=True)
    seg = c.build_segment(str(tmp_path / "p.seg"))
    db = Database(seg)
    l = _lib.lib()
    good = [plan(db, Query(t), 0, 10) for t in ("a", "b", "c")] + [plan(db, Query("OR", ["a", "c"]), 0, 10)]
    phrase = plan(db, Query("PHRASE", ["a", "b"]), 0, 10)
    assert phrase.phrase_active

    def call(plans, under=None, n=None, null_plans=False, null_out=False, handle=None):
        m = len(plans)
        arr = (_lib.Query * max(1, m))(*plans)
        hs = (C.c_void_p * max(1, m))(*([0xDEAD0] * max(1, m)))          # what an error must overwrite with NULL
        nd = (C.c_uint64 * max(1, m))()
        rc = l.xgm_filter_build_query_batch(handle or db._h, None if null_plans else arr, m if n is None else n, under._h if under is not None else None,
                                            None if null_out else hs, nd)
        return rc, list(hs), list(nd)

    def good_call():
        rc, hs, nd = call(good)
        assert rc == 0 and all(hs) and nd == [3, 3, 2, 3]
        for h in hs:
            l.xgm_filter_free(C.c_void_p(h))

    good_call()
    # an active positional plan at index 3 of 5: declined as a whole, the text names the index
    rc, hs, _ = call(good[:3] + [phrase] + good[3:])
    assert rc == UNSUPPORTED and not any(hs) and b"plan 3" in l.xgm_last_error()
    with pytest.raises(_lib.XgmUnsupported):
        db.build_query_filters(good[:3] + [phrase] + good[3:])
    good_call()
    # a term id beyond the dictionary: the first bad plan decides (index 1 is invalid, index 2 unsupported)
    bad = plan(db, Query("b"), 0, 10)
    bad.terms[0].term_id = db._info.n_terms
    rc, hs, _ = call([good[0], bad, phrase])
    assert rc == INVALID and not any(hs) and b"plan 1" in l.xgm_last_error()
    rc, hs, _ = call([good[0], phrase, bad])
    assert rc == UNSUPPORTED and not any(hs) and b"plan 1" in l.xgm_last_error()
    good_call()
    # a base filter of another index
    c2 = H.ManualCorpus({"a": [(1, 1), (70, 1)]}, {d: 6 for d in range(1, 71)}, positions=False)
    db2 = Database(c2.build_segment(str(tmp_path / "p2.seg")))
    other = db2.build_query_filter(plan(db2, Query("a"), 0, 10))
    rc, hs, _ = call(good, under=other)
    assert rc == INVALID and not any(hs)
    mine = db.build_query_filter(good[0])
    rc, hs, nd = call(good, under=mine)                                   # ... and its own index's is taken
    assert rc == 0 and nd == [3, 2, 2, 3]
    for h in hs:
        l.xgm_filter_free(C.c_void_p(h))
    # null arguments
    assert call(good, null_plans=True)[0] == INVALID
    assert call(good, null_out=True)[0] == INVALID
    assert l.xgm_filter_build_query_batch(None, (_lib.Query * 1)(good[0]), 1, None, (C.c_void_p * 1)(), None) == INVALID
    assert l.xgm_debug_filter_batch_info(None) != 0
    good_call()
    # an index without a device
    nodev = Database(seg, device=_lib.XGM_DEVICE_NONE)
    rc, hs, _ = call(good, handle=nodev._h)
    assert rc == NO_DEVICE and not any(hs)
    nodev.close()
    good_call()
    for f in (other, mine):
        f.close()
    db2.close()
    c2.close()
    db.close()
    c.close()
