"""A value-range filter as the whole query (include/xgm.h: xgm_search_range): the selection kernels of xgm_range.h against numpy at the sizes where
their tails, their tile loop and their digit passes can go wrong, against the filtered sorted search that is already pinned, and against the pinned
oracle's value order.

Every weight of a range-only tree is 0, so the reference orders by docid, or by (value, docid) under any of the three value sorts
(matcher/matcher.cc:415-430): the expected page is numpy's STABLE sort of the passing docids by the ordinal (forward) or by its complement (reverse).

The same file runs under the CPU emulation of the kernels (tests/test_emu_range.py against tests/emu/libxgm_emu.so)."""
import collections
import ctypes as C
import os
import random
import struct
import subprocess
import sys
import threading

import numpy as np
import pytest

import helpers as H
from xapiand_amd import Database, Query, _lib
from xapiand_amd.enquire import column_ord_range, plan, read_column_values, search_filtered, search_range

pytestmark = [pytest.mark.gpu]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = bool(os.environ.get("XGM_EMU_QUICK"))          # under emulation a workgroup barrier costs 256 fiber switches: small sizes
V, VR, RV = _lib.XGM_SORT_VALUE, _lib.XGM_SORT_VALUE_RELEVANCE, _lib.XGM_SORT_RELEVANCE_VALUE
ORD_MAX = _lib.XGM_ORD_MAX
MAX_K = _lib.XGM_MAX_K
N_C = 2 ** 23 + 10                                     # column C's n_distinct: 24 bits of key, three digit passes


def wbits(w):
    return struct.unpack("<Q", struct.pack("<d", w))[0]


def attach(db, slot, ords, n_distinct):
    o = np.ascontiguousarray(ords, dtype=np.uint32)
    _lib.check(_lib.lib().xgm_index_attach_column_ordinals(db._h, slot, o.ctypes.data_as(C.POINTER(C.c_uint32)), len(o), n_distinct))


def passes(cols, ranges):
    n = len(next(iter(cols.values())))
    ok = np.ones(n, dtype=bool)
    for slot, lo, hi in ranges:
        o = cols[slot]
        ok &= (o != 0) & (o >= lo) & (o <= hi)
    ok[0] = False
    return ok


def expected_page(ok, col, rev, k):
    """[(docid, ordinal)] of the first k passing documents under (value, docid): forward the smaller ordinal first and 0 before all, reverse the larger
    first and 0 last — the complement of the ordinal —, docid ascending among equals (a stable sort of the ascending docids); col None = docid order."""
    docs = np.nonzero(ok)[0].astype(np.uint32)
    if col is None:
        return [(int(d), 0) for d in docs[:k]]
    o = col[docs].astype(np.uint32)
    order = np.argsort(~o if rev else o, kind="stable")[:k]
    return [(int(docs[i]), int(o[i])) for i in order]


def check_page(got, hdr, counts, ok, col, rev, k, spy_col, n_spy, what):
    want = expected_page(ok, col, rev, k)
    n = int(ok.sum())
    assert [(d, o) for d, _, _, o in got] == want, what
    assert all(wbits(w) == 0 and m == 0 for _, w, m, _ in got), what
    assert (hdr.n_hits, hdr.matches_exact, hdr.max_weight_subqs_matched) == (min(k, n), n, 0), what
    assert wbits(hdr.max_attained) == 0 and wbits(hdr.max_possible) == 0, what
    if spy_col is None:
        assert counts is None
    else:
        assert counts == np.bincount(spy_col[ok], minlength=n_spy + 1).tolist() and sum(counts) == n, what


# ---- 1. against numpy, at the edges ----------------------------------------------------------------------------------------------

LASTDOCIDS = [1, 31, 32, 33, 2047, 2048, 2049, 4099]


def edge_columns(lastdocid):
    rng = np.random.RandomState(7000 + lastdocid)
    a = rng.randint(1, 10, size=lastdocid + 1).astype(np.uint32)          # A: 9 values, a fifth without one — the threshold value straddles k
    a[rng.rand(lastdocid + 1) < 0.2] = 0
    a[0] = 5                                                              # (ord[0] is unused: whatever it holds, docid 0 never passes)
    a[lastdocid] = 4
    b = np.zeros(lastdocid + 1, dtype=np.uint32)                          # B: every document its own ordinal — two digit passes at 4099
    b[1:] = rng.permutation(lastdocid) + 1
    c = rng.randint(1, N_C + 1, size=lastdocid + 1).astype(np.uint32)     # C: ordinals over [1, 2^23 + 10] — three digit passes
    c[1] = N_C
    c[lastdocid] = 1 if lastdocid > 1 else N_C
    return {0: a, 1: b, 2: c}, {0: 9, 1: lastdocid, 2: N_C}


def edge_filters(cols, lastdocid):
    rng = random.Random(lastdocid)
    lo = rng.randrange(1, 6)
    return [("drawn", [(0, lo, lo + rng.randrange(1, 4))]), ("empty", [(0, 5, 4)]), ("all", [(1, 1, ORD_MAX)]),
            ("last", [(1, int(cols[1][lastdocid]), int(cols[1][lastdocid]))]), ("first", [(1, int(cols[1][1]), int(cols[1][1]))])]


SORTS = [(None, 0, False)] + [(mode, slot, rev) for slot in (0, 1, 2) for rev in (False, True) for mode in (V, VR, RV)]


@pytest.mark.parametrize("lastdocid", LASTDOCIDS)
def test_range_vs_numpy(built, tmp_path, lastdocid):
    """Docids, ordinals, weight bits, weighted leaves, every header field and the spy's counts on column A — around the bitmap's word (32), the
    tile (2048), with more than one tile, with one, two and three digit passes, with pages the threshold value straddles."""
    c = H.ManualCorpus({"a": [(1, 1), (lastdocid, 2)] if lastdocid > 1 else [(1, 1)]}, {d: 5 + d % 7 for d in range(1, lastdocid + 1)}, positions=False)
    db = Database(c.build_segment(str(tmp_path / "r.seg")))
    assert db.get_lastdocid() == lastdocid
    cols, nd = edge_columns(lastdocid)
    for slot in cols:
        attach(db, slot, cols[slot], nd[slot])
    n_calls = n_straddled = 0
    seen = set()
    for kind, ranges in edge_filters(cols, lastdocid):
        ok = passes(cols, ranges)
        n = int(ok.sum())
        flt = db.build_filter(ranges)
        assert flt.n_docs == n, (kind, ranges)
        assert {"empty": n == 0, "all": n == lastdocid, "last": ok[lastdocid] and n == 1, "first": ok[1] and n == 1}.get(kind, True), kind
        seen.add(kind)
        ks = [1, 10, MAX_K, min(n + 7, MAX_K)]                           # (the last: above n_docs wherever XGM_MAX_K allows one)
        by_v = {}
        for si, (mode, slot, rev) in enumerate(SORTS):
            for ki, k in enumerate(ks):
                if QUICK and ki != si % len(ks):                          # the sort x k product cut to a diagonal
                    continue
                spy = (0, 9) if (si + ki) % 2 == 0 else None
                got, hdr, counts = search_range(db, flt, k, mode, slot, rev, spy=spy)
                what = (lastdocid, kind, mode, slot, rev, k, spy)
                col = cols[slot] if mode else None
                check_page(got, hdr, counts, ok, col, rev, k, cols[0] if spy else None, 9, what)
                n_calls += 1
                if mode and 0 < k < n:                                    # the k-th value is shared by documents beyond the page: the docid decides
                    o = np.sort(col[ok])[::-1 if rev else 1]
                    n_straddled += int(o[k - 1] == o[k])
                if mode == V:
                    by_v[(slot, rev, k)] = [h[:1] + h[3:] for h in got]
                elif mode and (slot, rev, k) in by_v:                     # VR and RV are V exactly
                    assert [h[:1] + h[3:] for h in got] == by_v[(slot, rev, k)], what
        flt.close()
    assert seen == {"drawn", "empty", "all", "last", "first"} and n_calls >= (90 if QUICK else 380)
    if lastdocid >= 2047:
        assert n_straddled > 0
    db.close()
    c.close()


@pytest.mark.parametrize("max_grid", ["1", "2"])
def test_range_tile_loop_with_a_capped_grid(built, max_grid):
    """XGM_RANGE_MAX_GRID (read once per process, hence the child): with one and two workgroups the tile kernels loop over the three tiles of 4099 documents."""
    if QUICK:
        pytest.skip("one emulated process per switch is not a quick run")
    env = dict(os.environ, XGM_RANGE_MAX_GRID=max_grid)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", "-k", "range_vs_numpy and 4099"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


# ---- 2. against the device path that is already pinned ---------------------------------------------------------------------------

def test_range_equals_filtered_search_of_a_term_in_every_document(built, tmp_path):
    """A term every document holds, pushed through the workgroup kernel under XGM_SORT_VALUE with the same filter, matches exactly the filter's documents:
    docids, ordinals, the match count and the spy's counts must be those of xgm_search_range."""
    n = 600 if QUICK else 3000
    c = H.ManualCorpus({"all": [(d, 1 + d % 3) for d in range(1, n + 1)], "some": [(d, 1) for d in range(2, n + 1, 7)]}, {d: 5 + d % 11 for d in range(1, n + 1)},
                       positions=False)
    db = Database(c.build_segment(str(tmp_path / "p.seg")))
    rng = np.random.RandomState(42)
    a = rng.randint(1, 10, size=n + 1).astype(np.uint32)
    a[rng.rand(n + 1) < 0.2] = 0
    b = np.zeros(n + 1, dtype=np.uint32)
    b[1:] = rng.permutation(n) + 1
    cols = {0: a, 1: b}
    attach(db, 0, a, 9)
    attach(db, 1, b, n)
    checked = 0
    for ranges in ([(0, 2, 6)], [(1, 1, ORD_MAX)], [(1, n // 3, 2 * n // 3), (0, 1, 8)]):
        flt = db.build_filter(ranges)
        assert flt.n_docs == int(passes(cols, ranges).sum()) > 100
        for k in (10, 300):
            p = plan(db, Query("OR", ["all"]), 0, k)
            for slot in (0, 1):
                for rev in (False, True):
                    want, whdr, wcounts = search_filtered(db, p, flt, V, slot, rev, spy=(0, 9))
                    for mode in (V, VR, RV):
                        got, hdr, counts = search_range(db, flt, k, mode, slot, rev, spy=(0, 9))
                        what = (ranges, k, slot, rev, mode)
                        assert [(d, o) for d, _, _, o in got] == [(d, o) for d, _, _, o in want] and len(got) == min(k, flt.n_docs), what
                        assert (hdr.n_hits, hdr.matches_exact) == (whdr.n_hits, whdr.matches_exact) and counts == wcounts, what
                        checked += 1
        flt.close()
    assert checked == 72
    db.close()
    c.close()


# ---- 3. against the pinned oracle's value order ------------------------------------------------------------------------------------

def write_column(corpus, slot, path):
    H.oracle_search_sorted(corpus, "OR", ["t1"], 0, 1, "V", slot, False)            # (makes the oracle index and its value slots)
    ol = H.olib()
    ol.xgo_write_value_column.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p]
    assert ol.xgo_write_value_column(corpus.oracle_index(), slot, path.encode()) == 0
    return path


class World:
    """One corpus, its three column files, their distinct values and ordinals, and the oracle's full rankings (computed once each)."""

    def __init__(self, tmp):
        self.c = H.Corpus(*((3000, 8000) if QUICK else (30000, 60000)))
        self.last = self.c.v.lastdocid
        self.paths, self.values, self.ords = {}, {}, {}
        for slot in range(3):
            p = write_column(self.c, slot, os.path.join(tmp, "col%d" % slot))
            self.paths[slot], self.values[slot] = p, read_column_values(p)
            self.ords[slot] = np.frombuffer(open(p, "rb").read(), dtype=np.uint32, count=self.last + 1, offset=24)
        self._full = {}

    def database(self, path, stripe_bits=0):
        db = Database(self.c.build_segment(path, stripe_bits=stripe_bits))
        for slot in range(3):
            db.attach_column(self.paths[slot])
        return db

    def full(self, term, slot, rev):
        """The oracle's ranking of every document holding `term` under the value sort: [(docid, weight, subqs, sort key bytes)]."""
        key = (term, slot, rev)
        if key not in self._full:
            self._full[key] = H.oracle_search_sorted(self.c, "OR", [term], 0, self.last, "V", slot, rev)[0]
        return self._full[key]


@pytest.fixture(scope="module")
def world(built, tmp_path_factory):
    w = World(str(tmp_path_factory.mktemp("range")))
    yield w
    w.c.close()


TERM = "t1"                                            # the corpus' most frequent term
ORACLE_SEED = 900


def draw_range_filter(w, rng):
    """A numeric interval on slot 1 sized to let a few hundred documents through, every third time narrowed by a category interval on slot 0."""
    width = rng.randrange(150000, 300000) if QUICK else rng.randrange(15000, 30000)
    a = rng.randrange(0, 1000000 - width)
    ranges = [(1,) + column_ord_range(w.paths[1], b"%06d" % a, b"%06d" % (a + width))]
    if rng.random() < 0.33:
        vals = w.values[0]
        ranges.append((0,) + column_ord_range(w.paths[0], vals[len(vals) // 8], vals[-1]))
    return ranges


@pytest.mark.parametrize("stripe_bits", [0, 10])
def test_range_value_order_vs_oracle(world, tmp_path, stripe_bits):
    """The oracle ranks the documents of a frequent term under the value sort; a filter letting fewer than 1024 documents through returns all of them,
    so those of its hits that hold the term must be exactly the oracle's ranking restricted to the filter, with the oracle's sort-key bytes."""
    w = world
    db = w.database(str(tmp_path / "o.seg"), stripe_bits)
    rng = random.Random(ORACLE_SEED + stripe_bits)
    n_cases = n_good = n_keys = 0
    for slot in range(3):
        for rev in (False, True):
            ranges = draw_range_filter(w, rng)
            ok = passes(w.ords, ranges)
            flt = db.build_filter(ranges)
            assert flt.n_docs == int(ok.sum())
            got, hdr, _ = search_range(db, flt, MAX_K, V, slot, rev)
            full = w.full(TERM, slot, rev)
            rank = {r[0]: i for i, r in enumerate(full)}
            kept = [h for h in got if h[0] in rank]
            assert [rank[h[0]] for h in kept] == sorted(rank[h[0]] for h in kept), (ranges, slot, rev)
            assert [w.values[slot][o - 1] if o else b"" for _, _, _, o in kept] == [full[rank[d]][3] for d, _, _, _ in kept], (ranges, slot, rev)
            if flt.n_docs <= MAX_K:                                       # the whole filter is on the page
                assert [h[0] for h in kept] == [r[0] for r in full if ok[r[0]]], (ranges, slot, rev)
            n_cases += 1
            n_good += 1 <= flt.n_docs < MAX_K and len(kept) >= 20
            n_keys += len(kept)
            flt.close()
    assert 2 * n_good >= n_cases == 6 and n_keys > 0, (n_good, n_cases)
    db.close()


# ---- 4. errors -----------------------------------------------------------------------------------------------------------------------

def test_range_argument_errors(built, tmp_path):
    c = H.ManualCorpus({"a": [(1, 1), (40, 1)]}, {d: 6 for d in range(1, 41)}, positions=False)
    db = Database(c.build_segment(str(tmp_path / "e.seg")))
    o = (np.arange(41, dtype=np.uint32) % 5).astype(np.uint32)
    attach(db, 0, o, 4)
    flt = db.build_filter([(0, 2, 3)])
    l = _lib.lib()
    hits, ords, hdr, counts = (_lib.Hit * 8)(), (C.c_uint32 * 8)(), _lib.ResultHdr(), (C.c_uint32 * 5)()
    call = lambda idx, f, h, hd, k=8: l.xgm_search_range(idx, f, None, k, h, ords, C.byref(hd) if hd is not None else None, -1, None, 0)
    for args in ((None, flt._h, hits, hdr), (db._h, None, hits, hdr), (db._h, flt._h, None, hdr), (db._h, flt._h, hits, None)):
        assert call(*args) == _lib.XGM_E_INVALID, args
    for k in (0, MAX_K + 1):
        with pytest.raises(_lib.XgmError) as e:
            search_range(db, flt, k)
        assert e.value.code == _lib.XGM_E_INVALID, k
    for nc, cnt in ((4, counts), (6, counts), (5, None)):                  # not the spy column's number of counters; no counters
        assert l.xgm_search_range(db._h, flt._h, None, 8, hits, ords, C.byref(hdr), 0, cnt, nc) == _lib.XGM_E_INVALID, nc
    with pytest.raises(_lib.XgmUnsupported):                               # no column attached for the sort slot
        search_range(db, flt, 8, V, 3)
    with pytest.raises(_lib.XgmUnsupported):                               # ... for the spy slot
        search_range(db, flt, 8, V, 0, spy=(3, 4))
    with pytest.raises(_lib.XgmError) as e:
        search_range(db, flt, 8, 7, 0)
    assert e.value.code == _lib.XGM_E_INVALID
    # a filter remembers its index: another one declines it
    c2 = H.ManualCorpus({"a": [(1, 1), (50, 1)]}, {d: 6 for d in range(1, 51)}, positions=False)
    db2 = Database(c2.build_segment(str(tmp_path / "e2.seg")))
    with pytest.raises(_lib.XgmError) as e:
        search_range(db2, flt, 8)
    assert e.value.code == _lib.XGM_E_INVALID
    # ... and its own index takes it, hit_ord being optional: document d passes when d % 5 is 2 or 3
    assert l.xgm_search_range(db._h, flt._h, None, 8, hits, None, C.byref(hdr), 0, counts, 5) == 0
    assert [hits[i].docid for i in range(hdr.n_hits)] == [2, 3, 7, 8, 12, 13, 17, 18] and hdr.matches_exact == 16 and list(counts) == [0, 0, 8, 8, 0]
    flt.close()
    for x in (db2, db):
        x.close()
    c.close()
    c2.close()


# ---- 5. threads ------------------------------------------------------------------------------------------------------------------------

def test_range_from_many_threads(built, tmp_path):
    """8 threads, 20 searches each with their own k and sort, on one index and one filter: every answer is the single-threaded one."""
    n = 700 if QUICK else 5000
    c = H.ManualCorpus({"a": [(1, 1), (n, 1)]}, {d: 6 for d in range(1, n + 1)}, positions=False)
    db = Database(c.build_segment(str(tmp_path / "t.seg")))
    cols, _ = edge_columns(n)
    attach(db, 0, cols[0], 9)
    attach(db, 1, cols[1], n)
    flt = db.build_filter([(0, 2, 7)])
    hf = lambda h: (h.n_hits, h.matches_exact, wbits(h.max_attained), h.max_weight_subqs_matched, wbits(h.max_possible))
    jobs = [[(1 + (37 * (t * 20 + i)) % 300, *SORTS[(t + 3 * i) % 13], (0, 9) if i % 2 else None) for i in range(20)] for t in range(8)]
    run = lambda k, mode, slot, rev, spy: (lambda g, h, cn: (g, hf(h), cn))(*search_range(db, flt, k, mode, slot, rev, spy=spy))
    want = [[run(*j) for j in js] for js in jobs]
    got, errors = [None] * 8, []

    def work(t):
        try:
            got[t] = [run(*j) for j in jobs[t]]
        except Exception as e:               # noqa: BLE001 (reported below)
            errors.append(repr(e))
    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert got == want and len({len(g[0]) for gs in got for g in gs}) > 5
    flt.close()
    db.close()
    c.close()
