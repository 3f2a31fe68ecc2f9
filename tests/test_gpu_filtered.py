"""Value-range filters on the device (include/xgm.h: xgm_filter_build, xgm_search_filtered*): the bitmap kernel against numpy at the sizes
where its tail, its word assembly and its grid can go wrong, and filtered searches against the pinned oracle.

The oracle ranks the WHOLE match under any sort and writes the column files; dropping documents from a total order leaves the order of the
rest unchanged, so the expected answer of a filtered search is the oracle's full ranking, filtered by the column's ordinals, cut to the page.
A range node weighs 0.0 (ValueRangePostList::get_weight), so the surviving documents keep their weight bits.

The same file runs under the CPU emulation of the kernels (tests/test_emu_filtered.py against tests/emu/libxgm_emu.so)."""
import collections
import ctypes as C
import os
import random
import struct

import numpy as np
import pytest

import helpers as H
from xapiand_amd import Database, Query, _lib
from xapiand_amd.enquire import (column_ord_range, plan, read_column_values, search_filtered, search_filtered_batch, search_sorted, search_sorted_batch,
                                 search_sorted_spy)

pytestmark = [pytest.mark.gpu]

QUICK = bool(os.environ.get("XGM_EMU_QUICK"))          # under emulation a workgroup barrier costs 256 fiber switches: small sizes
MODES = {"V": _lib.XGM_SORT_VALUE, "VR": _lib.XGM_SORT_VALUE_RELEVANCE, "RV": _lib.XGM_SORT_RELEVANCE_VALUE, None: None}
ORD_MAX = _lib.XGM_ORD_MAX


def wbits(w):
    return struct.unpack("<Q", struct.pack("<d", w))[0]


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

    def full(self, q, mode, slot, rev):
        """The oracle's ranking of the whole match: [(docid, weight, subqs, sort key bytes)] (key b"" by relevance)."""
        nr = q.get("n_required", 0)
        key = (q["op"], tuple(q["terms"]), nr) + ((mode, slot, rev) if mode else (None,))
        if key not in self._full:
            if mode:
                rows, _ = H.oracle_search_sorted(self.c, q["op"], q["terms"], 0, self.last, mode, slot, rev, n_required=nr)
            else:
                rows, _ = H.oracle_search(self.c, q["op"], q["terms"], 0, self.last, n_required=nr)
                rows = [r + (b"",) for r in rows]
            self._full[key] = rows
        return self._full[key]

    def passes(self, ranges):
        ok = np.ones(self.last + 1, dtype=bool)
        for slot, lo, hi in ranges:
            o = self.ords[slot]
            ok &= (o != 0) & (o >= lo) & (o <= hi)
        ok[0] = False
        return ok

    def plan(self, db, q):
        return plan(db, Query(q["op"], q["terms"], n_required=q.get("n_required", 0)), q["first"], q["maxitems"])


@pytest.fixture(scope="module")
def world(built, tmp_path_factory):
    w = World(str(tmp_path_factory.mktemp("filtered")))
    yield w
    w.c.close()


def check_against_oracle(w, q, mode, slot, rev, ranges, got, hdr, counts=None, spy_slot=None):
    """got / hdr / counts of a filtered search against the oracle's full ranking filtered by the columns; returns (filtered, unfiltered) sizes."""
    what = (q, mode, slot, rev, ranges)
    full = w.full(q, mode, slot, rev)
    ok = w.passes(ranges)
    filtered = [r for r in full if ok[r[0]]]
    # the device returns the ranking from rank 0 (the caller drops `first`): the whole prefix is compared, the page [first, first + maxitems) with it
    prefix = filtered[:q["first"] + q["maxitems"]]
    assert [(d, wbits(x), m) for d, x, m, _ in got] == [(d, wbits(x), m) for d, x, m, _ in prefix], what
    if mode:
        assert [w.values[slot][o - 1] if o else b"" for _, _, _, o in got] == [k for _, _, _, k in prefix], what
    assert hdr.matches_exact == len(filtered), what
    if filtered:
        assert hdr.n_hits == len(prefix) > 0 and wbits(hdr.max_attained) == max(wbits(r[1]) for r in filtered), what
    else:
        assert hdr.n_hits == 0 and hdr.max_attained == 0.0 and got == [], what
    if counts is not None:
        cnt = collections.Counter(int(w.ords[spy_slot][r[0]]) for r in filtered)
        assert counts == [cnt.get(o, 0) for o in range(len(w.values[spy_slot]) + 1)], what
    return len(filtered), len(full)


# ---- 1. the mark kernel alone --------------------------------------------------------------------------------------------------

CLAUSE_SETS = [[(0, 1, ORD_MAX)], [(0, 4, 4)], [(1, 3, 7)], [(0, 6, 2)], [(0, 2, 8), (1, 3, 7)], [(1, 1, 5), (1, 4, 9)], [(0, 1, ORD_MAX), (1, 1, 9), (0, 3, 3), (1, 2, 8)]]


@pytest.mark.parametrize("lastdocid", [1, 31, 32, 33, 255, 256, 257, 2047, 2048, 4099])
def test_mark_kernel_bitmap_equals_numpy(built, tmp_path, lastdocid):
    """The bitmap word for word (the bits of the last word beyond lastdocid included), the count, bit 0 — around the word (32), the
    wave's round (256 documents), the workgroup's tile (2048) and with more than one tile."""
    c = H.ManualCorpus({"a": [(1, 1), (lastdocid, 2)] if lastdocid > 1 else [(1, 1)]}, {d: 5 + d % 7 for d in range(1, lastdocid + 1)}, positions=False)
    db = Database(c.build_segment(str(tmp_path / "m.seg")))
    assert db.get_lastdocid() == lastdocid
    rng = np.random.RandomState(lastdocid)
    ords = {}
    for slot in (0, 1):
        o = rng.randint(1, 10, size=lastdocid + 1).astype(np.uint32)
        o[rng.rand(lastdocid + 1) < 0.2] = 0
        o[0] = 5                                                        # ord[0] is unused: whatever it holds, docid 0 never passes
        o[lastdocid] = 4 if slot == 0 else 5                            # the last document passes most clause sets: the tail is looked at
        ords[slot] = o
        _lib.check(_lib.lib().xgm_index_attach_column_ordinals(db._h, slot, o.ctypes.data_as(C.POINTER(C.c_uint32)), lastdocid + 1, 9))
    n_words = (lastdocid + 32) // 32
    some = 0
    for ranges in CLAUSE_SETS:
        ok = np.ones(lastdocid + 1, dtype=bool)
        for slot, lo, hi in ranges:
            ok &= (ords[slot] != 0) & (ords[slot] >= lo) & (ords[slot] <= hi)
        ok[0] = False
        padded = np.zeros(n_words * 32, dtype=np.uint8)
        padded[:lastdocid + 1] = ok
        want = np.packbits(padded, bitorder="little").view("<u4")
        flt = db.build_filter(ranges)
        got = np.array(flt.words(), dtype=np.uint32)
        assert got.shape == want.shape and (got == want).all(), (lastdocid, ranges, np.nonzero(got != want)[0][:8])
        assert flt.n_docs == int(ok.sum()), (lastdocid, ranges)
        assert not (got[0] & 1)
        some += int(ok.sum())
        flt.close()
    assert some > 0
    db.close()
    c.close()


def test_filter_argument_errors(built, tmp_path):
    c = H.ManualCorpus({"a": [(1, 1), (40, 1)]}, {d: 6 for d in range(1, 41)}, positions=False)
    seg = c.build_segment(str(tmp_path / "e.seg"))
    db = Database(seg)
    o = np.arange(41, dtype=np.uint32) % 5
    _lib.check(_lib.lib().xgm_index_attach_column_ordinals(db._h, 0, o.ctypes.data_as(C.POINTER(C.c_uint32)), 41, 4))
    for bad in ([], [(0, 1, 2)] * 5, [(0, 0, 3)], [(0, 1, 2), (0, 0, ORD_MAX)]):
        with pytest.raises(_lib.XgmError) as e:
            db.build_filter(bad)
        assert e.value.code == _lib.XGM_E_INVALID, bad
    with pytest.raises(_lib.XgmUnsupported):                           # no column attached for slot 3
        db.build_filter([(0, 1, 2), (3, 1, 2)])
    flt = db.build_filter([(0, 2, 3)])
    assert flt.n_docs == int(((o[1:] >= 2) & (o[1:] <= 3)).sum())
    with pytest.raises(_lib.XgmError) as e:                            # the bitmap has ceil((lastdocid + 1) / 32) words, no other number
        w = (C.c_uint32 * 5)()
        _lib.check(_lib.lib().xgm_filter_read(flt._h, w, 5))
    assert e.value.code == _lib.XGM_E_INVALID
    # a filter remembers its lastdocid: another index declines it
    c2 = H.ManualCorpus({"a": [(1, 1), (50, 1)]}, {d: 6 for d in range(1, 51)}, positions=False)
    db2 = Database(c2.build_segment(str(tmp_path / "e2.seg")))
    p2 = plan(db2, Query("OR", ["a"]), 0, 10)
    with pytest.raises(_lib.XgmError) as e:
        search_filtered(db2, p2, flt)
    assert e.value.code == _lib.XGM_E_INVALID
    with pytest.raises(_lib.XgmError) as e:
        search_filtered_batch(db2, [p2, p2], flt)
    assert e.value.code == _lib.XGM_E_INVALID
    # ... and its own index takes it: document d passes when d % 5 is 2 or 3
    got, hdr, _ = search_filtered(db, plan(db, Query("OR", ["a"]), 0, 10), flt)
    assert [d for d, _, _, _ in got] == [] and hdr.matches_exact == 0           # 1 % 5 and 40 % 5 are outside [2, 3]
    flt.close()
    # an index without a device builds no filter
    nodev = Database(seg, device=_lib.XGM_DEVICE_NONE)
    with pytest.raises(_lib.XgmError) as e:
        nodev.build_filter([(0, 1, 2)])
    assert e.value.code == _lib.XGM_E_NO_DEVICE
    for x in (nodev, db2, db):
        x.close()
    c.close()
    c2.close()


# ---- 2. filtered searches against the pinned oracle ---------------------------------------------------------------------------------

def query_mix():
    n = (lambda full, quick: quick if QUICK else full)
    return (H.gen_term_queries("OR", n(12, 3), 3, 1, 400, maxitems=10, seed=51) + H.gen_term_queries("AND", n(12, 3), 2, 1, 60, maxitems=10, seed=52) +
            H.gen_sided_queries("AND_MAYBE", n(6, 2), 1, 2, 1, 200, maxitems=10, seed=53) + H.gen_sided_queries("AND_NOT", n(6, 2), 1, 2, 1, 200, maxitems=10, seed=54) +
            H.gen_term_queries("OR", n(6, 1), 5, 1, 3000, first=7, maxitems=93, seed=55) + H.gen_term_queries("AND", n(4, 1), 3, 1, 30, maxitems=300, seed=56))


def draw_clause(w, rng, slot):
    """A clause from BYTE bounds, as a hook would make it: slot 0 an interval of categories, slot 1 a numeric interval, slot 2 one digit."""
    vals = w.values[slot]
    if slot == 0:
        a, b = sorted(rng.sample(range(len(vals)), 2))
        if b - a < len(vals) // 4:
            b = min(len(vals) - 1, a + len(vals) // 3)
        begin, end = vals[a], vals[b]
    elif slot == 1:
        a = rng.randrange(0, 600000)
        begin, end = b"%06d" % a, b"%06d" % (a + rng.randrange(250000, 400000))
    else:
        begin = end = rng.choice(vals)
    lo, hi = column_ord_range(w.paths[slot], begin, end)
    return (slot, lo, hi)


@pytest.mark.parametrize("stripe_bits", [0, 10])
def test_filtered_searches_vs_oracle(world, tmp_path, stripe_bits):
    w = world
    db = w.database(str(tmp_path / "s.seg"), stripe_bits)
    rng = random.Random(300 + stripe_bits)
    n_items = n_cases = n_partial = n_spied = 0
    special = {"empty": 0, "all": 0}
    base = query_mix()
    for qi, q in enumerate(base):
        for rep in range(1 if QUICK else 2):
            mode, slot, rev = rng.choice([None, "V", "VR", "RV"]), rng.randrange(3), rng.random() < 0.5
            kind = "empty" if (qi, rep) == (1, 0) else "all" if (qi, rep) == (2, 0) else "drawn"
            if kind == "empty":                                          # begin > end: lo_ord > hi_ord, nothing passes
                lo, hi = column_ord_range(w.paths[0], w.values[0][-1], w.values[0][0])
                assert lo > hi
                ranges = [(0, lo, hi)]
            elif kind == "all":                                          # OP_VALUE_GE "" on the slot every document has a value in
                lo, hi = column_ord_range(w.paths[2], b"", None)
                assert (lo, hi) == (1, ORD_MAX) and (w.ords[2][1:] != 0).all()
                ranges = [(2, lo, hi)]
            else:
                ranges = [draw_clause(w, rng, s) for s in rng.sample(range(3), 2 if rng.random() < 0.3 else 1)]
            flt = db.build_filter(ranges)
            assert flt.n_docs == int(w.passes(ranges).sum()), ranges
            spy = None
            if (qi + rep) % 3 == 0:
                spy_slot = (slot + 1 + rng.randrange(2)) % 3            # a slot other than the sort's
                spy = (spy_slot, len(w.values[spy_slot]))
                n_spied += 1
            got, hdr, counts = search_filtered(db, w.plan(db, q), flt, MODES[mode], slot, rev, spy=spy)
            nf, nu = check_against_oracle(w, q, mode, slot, rev, ranges, got, hdr, counts, spy[0] if spy else None)
            assert hdr.max_possible == w.plan(db, q).max_possible
            flt.close()
            if kind == "drawn":
                n_cases += 1
                n_partial += 0 < nf < nu
            else:
                special[kind] += 1
                assert nf == (0 if kind == "empty" else nu)
            n_items += len(got)
    assert special["empty"] >= 1 and special["all"] >= 1
    assert 2 * n_partial >= n_cases > 0, (n_partial, n_cases)
    assert n_items > (60 if QUICK else 500) and n_spied > 0
    db.close()


# ---- 3. a batch under one filter == the single searches ---------------------------------------------------------------------------

def test_filtered_batch_equals_single_searches_and_the_oracle(world, tmp_path):
    w = world
    db = w.database(str(tmp_path / "b.seg"))
    n = (lambda full, quick: quick if QUICK else full)
    base = (H.gen_term_queries("OR", n(28, 6), 3, 1, 400, maxitems=10, seed=151) + H.gen_term_queries("AND", n(24, 5), 2, 1, 60, maxitems=10, seed=152) +
            H.gen_sided_queries("AND_MAYBE", n(8, 2), 1, 2, 1, 200, maxitems=10, seed=153) + H.gen_sided_queries("AND_NOT", n(8, 2), 1, 2, 1, 200, maxitems=10, seed=154) +
            H.gen_term_queries("OR", n(6, 1), 5, 1, 3000, first=7, maxitems=33, seed=155) + H.gen_term_queries("AND", n(4, 1), 1, 1, 30, maxitems=20, seed=156))
    assert len(base) >= (16 if QUICK else 64)
    plans = [w.plan(db, q) for q in base]
    ranges = [(1,) + column_ord_range(w.paths[1], b"150000", b"800000"), (2,) + column_ord_range(w.paths[2], b"1", None)]
    flt = db.build_filter(ranges)
    assert 0 < flt.n_docs == int(w.passes(ranges).sum()) < w.last
    hf = lambda h: (h.n_hits, h.matches_exact, wbits(h.max_attained), h.max_weight_subqs_matched, wbits(h.max_possible))
    checked = dropped = 0
    for mode, slot, rev, spy in (("VR", 0, True, (2, len(w.values[2]))), (None, 0, False, None)):
        res = search_filtered_batch(db, plans, flt, MODES[mode], slot, rev, spy=spy)
        assert len(res) == len(base)
        for qi, (q, p, (got, hdr, counts)) in enumerate(zip(base, plans, res)):
            one, ohdr, ocounts = search_filtered(db, p, flt, MODES[mode], slot, rev, spy=spy)
            assert got == one and hf(hdr) == hf(ohdr) and counts == ocounts, (q, mode)
            if spy:
                assert sum(counts) == hdr.matches_exact, q
            if qi % 5 == 0:
                nf, nu = check_against_oracle(w, q, mode, slot, rev, ranges, got, hdr, counts, spy[0] if spy else None)
                dropped += nu - nf
                checked += 1
    assert checked >= (8 if QUICK else 26) and dropped > 0
    flt.close()
    db.close()


# ---- 4. nothing existing moves ------------------------------------------------------------------------------------------------------

def test_unfiltered_searches_do_not_move_and_an_all_pass_filter_changes_nothing(world, tmp_path):
    w = world
    db = w.database(str(tmp_path / "n.seg"), stripe_bits=10)
    qs = (H.gen_term_queries("OR", 3 if QUICK else 8, 3, 1, 400, maxitems=10, seed=251) + H.gen_term_queries("AND", 3 if QUICK else 6, 2, 1, 60, maxitems=10, seed=252) +
          H.gen_sided_queries("AND_NOT", 2 if QUICK else 6, 1, 2, 1, 200, maxitems=10, seed=253))
    if not QUICK:
        assert len(qs) == 20
    plans = [w.plan(db, q) for q in qs]
    nd = len(w.values[1])
    hf = lambda h: (h.n_hits, h.matches_exact, wbits(h.max_attained), h.max_weight_subqs_matched, wbits(h.max_possible))

    def snapshot():
        out = []
        for p in plans:
            got, hdr = search_sorted(db, p, MODES["VR"], 0, False)
            sgot, shdr, counts = search_sorted_spy(db, p, MODES["V"], 2, True, 1, nd)
            out.append((got, hf(hdr), sgot, hf(shdr), counts))
        out.append([(got, hf(hdr)) for got, hdr in search_sorted_batch(db, plans, MODES["RV"], 1, True)])
        return out
    before = snapshot()
    flt = db.build_filter([draw_clause(w, random.Random(5), 1)])
    for p in plans[:4]:
        search_filtered(db, p, flt, MODES["V"], 0, False, spy=(1, nd))
    search_filtered_batch(db, plans, flt)
    flt.close()
    assert snapshot() == before
    # an all-pass filter: slot 2, where every document has a value
    assert (w.ords[2][1:] != 0).all()
    every = db.build_filter([(2, 1, ORD_MAX)])
    assert every.n_docs == w.last
    for p in plans:
        for mode, slot, rev in (("V", 1, False), ("RV", 0, True)):
            got, hdr = search_sorted(db, p, MODES[mode], slot, rev)
            fgot, fhdr, _ = search_filtered(db, p, every, MODES[mode], slot, rev)
            assert fgot == got and hf(fhdr) == hf(hdr)
        sgot, shdr, counts = search_sorted_spy(db, p, MODES["V"], 2, True, 1, nd)
        fgot, fhdr, fcounts = search_filtered(db, p, every, MODES["V"], 2, True, spy=(1, nd))
        assert fgot == sgot and hf(fhdr) == hf(shdr) and fcounts == counts and sum(fcounts) == shdr.matches_exact
    for (got, hdr), (fgot, fhdr, _) in zip(search_sorted_batch(db, plans, MODES["VR"], 2, False), search_filtered_batch(db, plans, every, MODES["VR"], 2, False)):
        assert fgot == got and hf(fhdr) == hf(hdr)
    every.close()
    db.close()
