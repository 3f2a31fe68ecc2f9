"""The pair spy (include/xgm.h: xgm_filter_count_pairs): for a filter's documents, every distinct (ordinal in slot A, ordinal in slot B) with its
number of documents — the kernels of xgm_pairs.h against numpy at the sizes where their tails, their tile loop and their three paths (counters in
LDS, counters by global atomics, the open-addressing table) can go wrong, and against the one-slot spy of xgm_search_range that is already pinned.

The expected answer is np.unique over the stacked ordinals of the passing docids: its lexicographic order is the (ord_a, ord_b) order.
xgm_debug_pairs_info says which path answered, so every case also checks that it ran the path it is there for.

The same file runs under the CPU emulation of the kernels (tests/test_emu_pairs.py against tests/emu/libxgm_emu.so)."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import helpers as H
from test_gpu_range import LASTDOCIDS, N_C, attach, edge_columns, edge_filters, passes
from xapiand_amd import Database, _lib
from xapiand_amd.enquire import count_pairs, search_range

pytestmark = [pytest.mark.gpu]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = bool(os.environ.get("XGM_EMU_QUICK"))          # under emulation a workgroup barrier costs 256 fiber switches: fewer calls
LDS_MAX = 8192                                         # kRangeSpyLds
DENSE_MAX = 1 << 22                                    # kPairDenseMax, unless XGM_PAIRS_DENSE_MAX says otherwise (read once per process)
if os.environ.get("XGM_PAIRS_DENSE_MAX"):
    DENSE_MAX = min(max(int(os.environ["XGM_PAIRS_DENSE_MAX"]), 0), 1 << 28)
LDS, GLOBAL, TABLE = 1, 2, 3
POISON = 0xA5A5A5A5


def make_db(tmp_path, lastdocid, name="p.seg"):
    c = H.ManualCorpus({"a": [(1, 1), (lastdocid, 2)] if lastdocid > 1 else [(1, 1)]}, {d: 5 + d % 7 for d in range(1, lastdocid + 1)}, positions=False)
    db = Database(c.build_segment(str(tmp_path / name)))
    assert db.get_lastdocid() == lastdocid
    return c, db


def expected_pairs(ok, a, b):
    """[(ord_a, ord_b, count)] of the passing documents, ascending by (ord_a, ord_b)"""
    docs = np.nonzero(ok)[0]
    if docs.size == 0:
        return []
    u, n = np.unique(np.stack([a[docs], b[docs]]), axis=1, return_counts=True)
    return list(zip(u[0].tolist(), u[1].tolist(), n.tolist()))


def expected_path(n_a, n_b, n_docs):
    """(path, counters or table slots) the host picks for two columns of n_a / n_b distinct values under a filter of n_docs documents"""
    p = (n_a + 1) * (n_b + 1)
    if p <= DENSE_MAX:
        return (LDS if p <= LDS_MAX else GLOBAL), p
    s = 1024
    while s < 2 * min(n_docs, p):
        s *= 2
    return TABLE, s


def raw(db, flt, slot_a, slot_b, cap):
    """One call with room for `cap` records in a poisoned buffer of cap + 1 → (n_pairs, the buffer as rows of four words)"""
    buf = np.full((cap + 1, 4), POISON, dtype=np.uint32)
    n = C.c_uint64(12345)
    _lib.check(_lib.lib().xgm_filter_count_pairs(db._h, flt._h, slot_a, slot_b, buf.ctypes.data_as(C.POINTER(_lib.PairCount)), cap, C.byref(n)))
    return n.value, buf


def pairs_info():
    out = (C.c_uint64 * 4)()
    assert _lib.lib().xgm_debug_pairs_info(out) == 0
    return list(out)


def check_call(db, flt, slot_a, slot_b, want, n_docs, nd, what, short_caps=True):
    """The full answer (pairs, counts, order, their sum, reserved, the record behind the last one untouched, the path that ran), then — short_caps —
    cap = 0 and cap = n_pairs - 1: n_pairs reported, nothing written."""
    n, buf = raw(db, flt, slot_a, slot_b, len(want))
    assert n == len(want), what
    assert [tuple(r) for r in buf[:n, :3].tolist()] == want, what
    assert not buf[:n, 3].any() and (buf[n] == POISON).all(), what
    assert int(buf[:n, 2].sum()) == n_docs == sum(w[2] for w in want), what
    assert sorted(want) == want and len(set(w[:2] for w in want)) == len(want), what
    if n_docs:
        path, slots = expected_path(nd[slot_a], nd[slot_b], n_docs)
        assert pairs_info()[:3] == [path, slots, n], what
    if slot_a == slot_b:
        assert all(w[0] == w[1] for w in want), what
    for cap in ({0, max(n - 1, 0)} if short_caps else ()):
        if cap < n:
            m, b2 = raw(db, flt, slot_a, slot_b, cap)
            assert m == n and (b2 == POISON).all(), (what, cap)
    return n


# ---- 1. against numpy, at the edges ----------------------------------------------------------------------------------------------

A, B, CC = 0, 1, 2                                     # edge_columns: A 9 values and a fifth without one, B every document its own, C over [1, 2^23 + 10]
SLOT_PAIRS = [(A, A), (A, B), (B, A), (A, CC), (CC, A), (B, CC), (CC, B)]


def named_path(sa, sb, lastdocid):
    """The path each case is there for: A x A has 100 counters, A x B 10 (lastdocid + 1) — in LDS up to 800 documents, 20 480 and more from 2047 on —,
    anything with C more than 2^22; XGM_PAIRS_DENSE_MAX=0 sends everything through the table."""
    if CC in (sa, sb) or DENSE_MAX == 0:
        return TABLE
    if sa == sb:
        return LDS
    return LDS if lastdocid <= 800 else GLOBAL


@pytest.mark.parametrize("lastdocid", LASTDOCIDS)
def test_pairs_vs_numpy(built, tmp_path, lastdocid):
    """Around the bitmap's word (32), the tile (2048), with three tiles; A x A in LDS counters, A x B in LDS counters up to 800 documents and by global
    atomics at 4099 (P = 41 000), A x C and B x C through the table (P > 2^22 with columns of at most 4100 entries); each pair of slots also swapped;
    under a drawn, an empty, an all-pass, a first-document-only and a last-document-only filter."""
    c, db = make_db(tmp_path, lastdocid)
    cols, nd = edge_columns(lastdocid)
    for slot in cols:
        attach(db, slot, cols[slot], nd[slot])
    seen, paths, n_calls = set(), set(), 0
    for fi, (kind, ranges) in enumerate(edge_filters(cols, lastdocid)):
        ok = passes(cols, ranges)
        n_docs = int(ok.sum())
        flt = db.build_filter(ranges)
        assert flt.n_docs == n_docs, (kind, ranges)
        seen.add(kind)
        for pi, (sa, sb) in enumerate(SLOT_PAIRS):
            if QUICK and lastdocid == 2049 and sa > sb:                  # (the emulation's minute: 2049 keeps the unswapped runs, 4099 runs them all)
                continue
            want = expected_pairs(ok, cols[sa], cols[sb])
            what = (lastdocid, kind, sa, sb)
            check_call(db, flt, sa, sb, want, n_docs, nd, what, short_caps=not QUICK or (fi + pi) % 3 == 0)
            assert count_pairs(db, flt, sa, sb) == want, what
            n_calls += 1
            if n_docs:
                paths.add((sa, sb, expected_path(nd[sa], nd[sb], n_docs)[0]))
        flt.close()
    assert seen == {"drawn", "empty", "all", "last", "first"} and n_calls >= 20
    assert {(sa, sb) for sa, sb, _ in paths} == {sp for sp in SLOT_PAIRS if not (QUICK and lastdocid == 2049 and sp[0] > sp[1])}
    for sa, sb, path in paths:
        assert path == named_path(sa, sb, lastdocid), (sa, sb, path)
    db.close()
    c.close()


# ---- 2. the table under pressure ---------------------------------------------------------------------------------------------------

def test_pairs_table_under_pressure(built, tmp_path):
    """B x C at 4099 documents, every pair distinct: 600 passing documents in a table of 2048 slots (load 0.29), 1024 in 2048 (the full 0.5 the sizing
    allows); then two constant columns with a large n_distinct: every passing document on ONE pair, every atomic on one slot."""
    lastdocid = 4099
    c, db = make_db(tmp_path, lastdocid)
    cols, nd = edge_columns(lastdocid)
    cols[3] = np.full(lastdocid + 1, 7, dtype=np.uint32)
    cols[4] = np.full(lastdocid + 1, N_C - 3, dtype=np.uint32)
    nd[3] = nd[4] = N_C
    for slot in cols:
        attach(db, slot, cols[slot], nd[slot])
    for n_pass in (600, 1024):
        ranges = [(B, 1, n_pass)]                                         # B is a permutation: exactly n_pass documents
        ok = passes(cols, ranges)
        flt = db.build_filter(ranges)
        assert flt.n_docs == n_pass == int(ok.sum())
        for sa, sb in ((B, CC), (CC, B)):
            want = expected_pairs(ok, cols[sa], cols[sb])
            assert len(want) == n_pass
            check_call(db, flt, sa, sb, want, n_pass, nd, (n_pass, sa, sb))
            assert pairs_info()[:2] == [TABLE, 2048] or DENSE_MAX != 1 << 22
        flt.close()
    for ranges in ([(B, 1, _lib.XGM_ORD_MAX)], [(A, 2, 6)]):
        ok = passes(cols, ranges)
        flt = db.build_filter(ranges)
        want = [(7, N_C - 3, int(ok.sum()))]
        check_call(db, flt, 3, 4, want, int(ok.sum()), nd, ranges)
        assert check_call(db, flt, 4, 3, [(N_C - 3, 7, int(ok.sum()))], int(ok.sum()), nd, ranges) == 1
        assert pairs_info()[0] == TABLE or DENSE_MAX != 1 << 22
        flt.close()
    db.close()
    c.close()


# ---- 3. the table equals the counters; 4. the tile loop ---------------------------------------------------------------------------

def run_child(env, select, n_passed):
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", "-k", select],
                       cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "%d passed" % n_passed in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_pairs_table_equals_counters(built):
    """XGM_PAIRS_DENSE_MAX=0 (read once per process, hence the child) sends the pairs the counters answer above — A x A, A x B — through the table, at 31
    documents and at 4099: the same numpy answer, so the same records, in the same order (the host's sort); the child checks that the table ran."""
    run_child({"XGM_PAIRS_DENSE_MAX": "0"}, "pairs_vs_numpy and (31 or 4099)", 2)


@pytest.mark.parametrize("max_grid", ["1", "2"])
def test_pairs_tile_loop_with_a_capped_grid(built, max_grid):
    """XGM_RANGE_MAX_GRID: with one and two workgroups the tally kernel loops over the three tiles of 4099 documents, the count and place kernels over
    the 21 chunks of A x B's 41 000 counters."""
    run_child({"XGM_RANGE_MAX_GRID": max_grid}, "pairs_vs_numpy and 4099", 1)


# ---- 5. against the one-slot spy that is already pinned ------------------------------------------------------------------------------

def test_pairs_marginals_equal_the_one_slot_spy(built, tmp_path):
    """For each a, the sum over b of the pair counts is xgm_search_range's spy count of a on slot_a under the same filter, and likewise for b — under
    value filters and under a list-kind filter (XGM_RANGE_LIST on a list column)."""
    lastdocid = 700 if QUICK else 4099
    c, db = make_db(tmp_path, lastdocid)
    cols, nd = edge_columns(lastdocid)
    for slot in cols:
        attach(db, slot, cols[slot], nd[slot])
    rng = np.random.RandomState(11)
    n_el = rng.randint(0, 4, size=lastdocid + 1)                          # a list column on slot 5: 0 .. 3 elements of 1 .. 9 per document
    n_el[0] = 0
    off = np.concatenate([[0], np.cumsum(n_el)]).astype(np.uint32)
    elem = np.concatenate([np.sort(rng.choice(np.arange(1, 10), size=k, replace=False)) for k in n_el] + [np.zeros(0, dtype=np.int64)]).astype(np.uint32)
    db.attach_list_column_arrays(5, off, elem, 9)
    checked = 0
    for ranges in ([(A, 2, 6)], [(B, 1, _lib.XGM_ORD_MAX)], [(B, lastdocid // 3, 2 * lastdocid // 3), (A, 1, 8)], [(5, 4, 6, _lib.XGM_RANGE_LIST)],
                   [(5, 2, 3, _lib.XGM_RANGE_LIST), (A, 1, 9)]):
        flt = db.build_filter(ranges)
        assert flt.n_docs > 50, ranges
        spy = {s: search_range(db, flt, 1, spy=(s, nd[s]))[2] for s in (A, B)}
        assert all(sum(v) == flt.n_docs for v in spy.values())
        for sa, sb in ((A, B), (B, A), (A, A), (A, CC), (CC, B)):
            got = count_pairs(db, flt, sa, sb)
            assert sum(n for _, _, n in got) == flt.n_docs
            for side, slot in ((0, sa), (1, sb)):
                if slot in spy:
                    marg = np.zeros(nd[slot] + 1, dtype=np.int64)
                    for p in got:
                        marg[p[side]] += p[2]
                    assert marg.tolist() == spy[slot], (ranges, sa, sb, side)
                    checked += 1
        flt.close()
    assert checked == 5 * 8
    db.close()
    c.close()


# ---- 6. errors, threads ----------------------------------------------------------------------------------------------------------------

def test_pairs_argument_errors(built, tmp_path):
    """Every row of the error table but XGM_E_NOMEM, which only an exhausted device gives (no test provokes that on a shared machine)."""
    c, db = make_db(tmp_path, 40, "e.seg")
    o = (np.arange(41, dtype=np.uint32) % 5).astype(np.uint32)
    attach(db, 0, o, 4)
    attach(db, 1, o, 0xFFFFFFFF)                                         # the table's empty marker would be a pair
    flt = db.build_filter([(0, 2, 3)])
    l = _lib.lib()
    buf, n = (_lib.PairCount * 8)(), C.c_uint64(77)
    call = lambda idx, f, sa, sb, p, cap, np_: l.xgm_filter_count_pairs(idx, f, sa, sb, p, cap, C.byref(np_) if np_ is not None else None)
    for args in ((None, flt._h, 0, 0, buf, 8, n), (db._h, None, 0, 0, buf, 8, n), (db._h, flt._h, 0, 0, buf, 8, None), (db._h, flt._h, 0, 0, None, 8, n)):
        assert call(*args) == _lib.XGM_E_INVALID, args
    # a filter remembers its index: another one declines it
    c2, db2 = make_db(tmp_path, 50, "e2.seg")
    attach(db2, 0, (np.arange(51, dtype=np.uint32) % 5).astype(np.uint32), 4)
    assert call(db2._h, flt._h, 0, 0, buf, 8, n) == _lib.XGM_E_INVALID
    for sa, sb in ((0, 3), (3, 0), (3, 3)):                                # a slot without a plain column
        assert call(db._h, flt._h, sa, sb, buf, 8, n) == _lib.XGM_UNSUPPORTED, (sa, sb)
    for sa, sb in ((0, 1), (1, 0), (1, 1)):                                # n_distinct == 0xFFFFFFFF
        assert call(db._h, flt._h, sa, sb, buf, 8, n) == _lib.XGM_UNSUPPORTED, (sa, sb)
    db.attach_list_column_arrays(6, np.zeros(42, dtype=np.uint32), np.zeros(0, dtype=np.uint32), 4)
    assert call(db._h, flt._h, 0, 6, buf, 8, n) == _lib.XGM_UNSUPPORTED  # a list column is not a plain column
    nodev = Database(str(tmp_path / "e.seg"), device=_lib.XGM_DEVICE_NONE)
    assert call(nodev._h, flt._h, 0, 0, buf, 8, n) == _lib.XGM_E_NO_DEVICE
    nodev.close()
    # ... and its own index takes it, pairs being optional when cap is 0: document d passes when d % 5 is 2 or 3
    assert call(db._h, flt._h, 0, 0, None, 0, n) == 0 and n.value == 2
    assert call(db._h, flt._h, 0, 0, buf, 8, n) == 0 and n.value == 2
    assert [(buf[i].ord_a, buf[i].ord_b, buf[i].count, buf[i].reserved) for i in range(2)] == [(2, 2, 8, 0), (3, 3, 8, 0)]
    empty = db.build_filter([(0, 3, 2)])
    n.value = 77
    assert call(db._h, empty._h, 0, 0, buf, 8, n) == 0 and n.value == 0 and count_pairs(db, empty, 0, 0) == []
    for f in (empty, flt):
        f.close()
    for x in (db2, db):
        x.close()
    c.close()
    c2.close()


def test_pairs_from_many_threads(built, tmp_path):
    """8 threads, 12 calls each over all three paths, on one index and one filter: every answer is the single-threaded one."""
    lastdocid = 700 if QUICK else 4099
    c, db = make_db(tmp_path, lastdocid, "t.seg")
    cols, nd = edge_columns(lastdocid)
    for slot in cols:
        attach(db, slot, cols[slot], nd[slot])
    flt = db.build_filter([(A, 2, 7)])
    ok = passes(cols, [(A, 2, 7)])
    want = {sp: expected_pairs(ok, cols[sp[0]], cols[sp[1]]) for sp in SLOT_PAIRS}
    assert all(count_pairs(db, flt, *sp) == want[sp] for sp in SLOT_PAIRS)
    jobs = [[SLOT_PAIRS[(t + 3 * i) % len(SLOT_PAIRS)] for i in range(12)] for t in range(8)]
    got, errors = [None] * 8, []

    def work(t):
        try:
            got[t] = [count_pairs(db, flt, *sp) for sp in jobs[t]]
        except Exception as e:               # noqa: BLE001 (reported below)
            errors.append(repr(e))
    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert got == [[want[sp] for sp in js] for js in jobs]
    flt.close()
    db.close()
    c.close()
