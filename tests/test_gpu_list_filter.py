"""Range filters over multi-valued slots on the device (include/xgm.h: xgm_index_attach_list_column*, XGM_RANGE_LIST / _LIST_GE / _LIST_LE):
the bitmap of xgm_filter_mark_lists_kernel against a Python restatement, in ordinals, of the three insideRange() bodies of the reference
(src/multivalue/range.cc:352-368 MultipleValueRange, 484-494 MultipleValueGE, 609-619 MultipleValueLE) — `e >= start` is e >= lo, `e <= end` is
e <= hi, the list in STORED order — and filtered searches against the pinned oracle's full ranking, filtered by the same restatement (the argument
of tests/test_gpu_filtered.py: dropping documents from a total order leaves the order of the rest unchanged, a range node weighs 0.0).

Lists are attached from memory (Database.attach_list_column_arrays).  The same file runs under the CPU emulation of the kernels with guard pages
behind every device buffer (tests/test_emu_list_filter.py): a read of ext beyond a list's last ordinal faults there."""
import ctypes as C
import random

import numpy as np
import pytest

import helpers as H
import test_gpu_filtered as F
from xapiand_amd import Database, _lib
from xapiand_amd.enquire import search_filtered, search_range, search_sorted

pytestmark = [pytest.mark.gpu]

QUICK = F.QUICK
ORD_MAX = _lib.XGM_ORD_MAX
VALUE, LIST, GE, LE = _lib.XGM_RANGE_VALUE, _lib.XGM_RANGE_LIST, _lib.XGM_RANGE_LIST_GE, _lib.XGM_RANGE_LIST_LE
U32 = C.POINTER(C.c_uint32)


def inside(kind, data, lo, hi):
    """range.cc:352-368 / 484-494 / 609-619 on a document's element ordinals in stored order."""
    if not data:                                                       # data.empty()
        return False
    if kind == GE:
        return data[-1] >= lo                                          # data.back() >= start
    if kind == LE:
        return data[0] <= hi                                           # data.front() <= end
    if hi < data[0] or lo > data[-1]:                                  # end < data.front() || start > data.back()
        return False
    for e in data:
        if e >= lo:                                                    # value_ >= start
            return e <= hi                                             # return value_ <= end
    return False


def expected(lastdocid, ranges, plain, lists):
    """One bool per docid 0 .. lastdocid: plain[slot] an array of ordinals, lists[slot] a list of lists; 3-tuples are XGM_RANGE_VALUE clauses."""
    ok = np.ones(lastdocid + 1, dtype=bool)
    for r in ranges:
        slot, lo, hi, kind = r if len(r) == 4 else r + (VALUE,)
        if kind == VALUE:
            o = plain[slot]
            ok &= (o != 0) & (o >= lo) & (o <= hi)
        else:
            ok &= np.array([inside(kind, l, lo, hi) for l in lists[slot]], dtype=bool)
    ok[0] = False
    return ok


def csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(l) for l in lists])
    return off, np.array([e for l in lists for e in l], dtype=np.uint32)


def words_of(ok):
    padded = np.zeros((len(ok) + 31) // 32 * 32, dtype=np.uint8)
    padded[:len(ok)] = ok
    return np.packbits(padded, bitorder="little").view("<u4")


def check_bitmap(db, ranges, ok, what):
    flt = db.build_filter(ranges)
    got, want = np.array(flt.words(), dtype=np.uint32), words_of(ok)
    assert got.shape == want.shape and (got == want).all(), (what, ranges, np.nonzero(got != want)[0][:8])
    assert flt.n_docs == int(ok.sum()), (what, ranges)
    flt.close()
    return int(ok.sum())


def manual_db(tmp_path, lastdocid, name="m.seg"):
    c = H.ManualCorpus({"a": [(1, 1), (lastdocid, 2)] if lastdocid > 1 else [(1, 1)]}, {d: 5 + d % 7 for d in range(1, lastdocid + 1)}, positions=False)
    db = Database(c.build_segment(str(tmp_path / name)))
    assert db.get_lastdocid() == lastdocid
    return c, db


def attach_plain(db, slot, o, n_distinct):
    o = np.ascontiguousarray(o, dtype=np.uint32)
    _lib.check(_lib.lib().xgm_index_attach_column_ordinals(db._h, slot, o.ctypes.data_as(U32), len(o), n_distinct))


# ---- 1. the bitmap, word for word ------------------------------------------------------------------------------------------------------

CLAUSE_SETS = [
    [(0, 3, 6, LIST)], [(0, 4, 0, GE)], [(1, 1, 5, LE)], [(0, 2, 5, VALUE)], [(1, 3, 7)],          # every kind alone (GE ignores hi, LE ignores lo)
    [(0, 6, 2, LIST)],                                                                            # lo > hi
    [(1, 4, ORD_MAX, LIST)], [(0, 1, ORD_MAX, LIST)],                                             # hi = XGM_ORD_MAX
    [(0, 2, 8, LIST), (0, 5, 0, GE)], [(1, 4, 6, LIST), (1, 1, 7, LE), (1, 2, 9, LIST)],          # list clauses on one slot
    [(0, 2, 8), (1, 3, 7, LIST)], [(1, 1, ORD_MAX, GE), (0, 4, 4, VALUE)],                         # list and plain mixed
    [(1, 1, 9, VALUE), (0, 3, 5, LIST), (1, 4, 1, GE), (0, 1, 6, LE)], [(0, 1, ORD_MAX), (1, 2, 8), (0, 3, 9), (1, 2, 8, LIST)],
]


@pytest.mark.parametrize("last_doc", ["multi", "empty"])
@pytest.mark.parametrize("lastdocid", [1, 31, 32, 33, 255, 256, 257, 2047, 2048, 4099])
def test_list_mark_kernel_bitmap_equals_the_restated_rules(built, tmp_path, lastdocid, last_doc):
    """Random lists of 0 .. 3 elements over 9 distinct values, unsorted and with duplicates, on two slots that ALSO carry plain columns; the last
    document multi-element (its list ends ext: nothing may be read behind it) or without elements (lastdocid 1, 33, 257 straddle a group of four
    with 1 document, 32, 256, 2048 with none before it in the group) — around the word (32), the wave's round (256), the tile (2048), two tiles."""
    c, db = manual_db(tmp_path, lastdocid)
    rng = np.random.RandomState(1000 + lastdocid)
    plain, lists = {}, {}
    for slot in (0, 1):
        o = rng.randint(1, 10, size=lastdocid + 1).astype(np.uint32)
        o[rng.rand(lastdocid + 1) < 0.2] = 0
        o[0] = 5
        plain[slot] = o
        attach_plain(db, slot, o, 9)
        ls = [[]] + [[int(x) for x in rng.randint(1, 10, size=rng.randint(0, 4))] for _ in range(lastdocid)]
        ls[lastdocid] = [] if last_doc == "empty" else ([3, 7, 4] if slot == 0 else [5, 5])
        lists[slot] = ls
        off, elem = csr(ls)
        db.attach_list_column_arrays(slot, off, elem, 9)
    some = 0
    for ranges in CLAUSE_SETS:
        some += check_bitmap(db, ranges, expected(lastdocid, ranges, plain, lists), (lastdocid, last_doc))
    assert some > 0
    db.close()
    c.close()


# ---- 2. long lists, all-multi and all-single columns -------------------------------------------------------------------------------------

def test_long_lists_among_single_valued_neighbours(built, tmp_path):
    """Documents of 2, 63, 64, 65 and 300 elements between single-valued ones: lanes of one wave walk lists of very different lengths, the loop is
    bounded by each list's own n.  Ascending lists (LIST = "some element inside") and shuffled ones (the first element at or above lo decides)."""
    lastdocid = 700
    c, db = manual_db(tmp_path, lastdocid)
    rng = random.Random(77)
    nd = 1000
    for variant in ("ascending", "shuffled"):
        ls = [[]] + [[rng.randrange(1, nd + 1)] for _ in range(lastdocid)]
        for d, n in ((5, 2), (6, 63), (7, 64), (64, 65), (65, 300), (130, 300), (131, 2), (258, 64), (699, 65), (700, 300)):
            l = rng.sample(range(1, nd + 1), n)
            ls[d] = sorted(l) if variant == "ascending" else l
        ls[300] = []
        off, elem = csr(ls)
        db.attach_list_column_arrays(2, off, elem, nd)
        longs = 0
        for ranges in ([(2, 400, 420, LIST)], [(2, 990, 0, GE)], [(2, 1, 10, LE)], [(2, 1, ORD_MAX, LIST)], [(2, 999, 1000, LIST)], [(2, 500, 500, LIST)],
                       [(2, 100, 900, LIST), (2, 200, 0, GE), (2, 1, 800, LE)]):
            ok = expected(lastdocid, ranges, {}, {2: ls})
            check_bitmap(db, ranges, ok, variant)
            longs += int(sum(ok[d] for d in (6, 7, 64, 65, 130, 258, 699, 700)))
        assert longs > 8
    db.close()
    c.close()


def test_all_multi_and_all_single_columns(built, tmp_path):
    lastdocid = 2500
    c, db = manual_db(tmp_path, lastdocid)
    rng = np.random.RandomState(3)
    multi = [[]] + [[int(x) for x in rng.randint(1, 10, size=rng.randint(2, 5))] for _ in range(lastdocid)]
    single = [[]] + [[int(x)] for x in rng.randint(1, 10, size=lastdocid)]
    o = np.array([0] + [l[0] for l in single[1:]], dtype=np.uint32)
    db.attach_list_column_arrays(0, *csr(multi), 9)
    db.attach_list_column_arrays(1, *csr(single), 9)
    attach_plain(db, 1, o, 9)
    for kind, lo, hi in ((LIST, 3, 6), (GE, 5, 0), (LE, 1, 4), (LIST, 7, 2), (LIST, 2, ORD_MAX)):
        assert check_bitmap(db, [(0, lo, hi, kind)], expected(lastdocid, [(0, lo, hi, kind)], {}, {0: multi}), "all multi") > 0 or lo > hi
        # every document single: the list clause is the plain kernel's filter of the same ordinals, word for word
        plo, phi = (1 if kind == LE else lo), (ORD_MAX if kind == GE else hi)
        fl, fp = db.build_filter([(1, lo, hi, kind)]), db.build_filter([(1, plo, phi)])
        assert fl.words() == fp.words() and fl.n_docs == fp.n_docs == int(((o >= plo) & (o <= phi) & (o != 0)).sum())
        fl.close()
        fp.close()
    db.close()
    c.close()


# ---- 3. stored order: the reference's rule, not "any element inside" --------------------------------------------------------------------------

def test_stored_order_decides_where_it_disagrees_with_any_element(built, tmp_path):
    cases = [([2, 9, 4], LIST, 3, 5, False),      # the first element >= 3 is 9, and 9 > 5 (4 lies inside: "any element" would pass)
             ([2, 4, 9], LIST, 3, 5, True),       # sorted: both rules pass
             ([9, 2], GE, 5, 0, False),           # back() is 2
             ([2, 9], GE, 5, 0, True),
             ([9, 2], LE, 1, 5, False),           # front() is 9
             ([2, 9], LE, 1, 5, True),
             ([9, 2, 4], LIST, 3, 5, False),      # front 9 > hi: no, whatever follows
             ([4, 4, 9, 4], LIST, 4, 4, True),    # duplicates kept
             ([3, 1, 1], LIST, 2, 5, False),      # lo > back()
             ([1, 6, 3], LIST, 2, 5, False)]      # 6 decides
    lastdocid = 40
    c, db = manual_db(tmp_path, lastdocid)
    for i, (data, kind, lo, hi, want) in enumerate(cases):
        assert inside(kind, data, lo, hi) == want, (data, kind)
        ls = [[]] + [[] for _ in range(lastdocid)]
        docs = (1, 7 + i, lastdocid)                                   # among empty neighbours, first and last document included
        for d in docs:
            ls[d] = data
        db.attach_list_column_arrays(3, *csr(ls), 9)                   # (attaching again replaces the slot's list column)
        flt = db.build_filter([(3, lo, hi, kind)])
        ok = expected(lastdocid, [(3, lo, hi, kind)], {}, {3: ls})
        assert [int(d) for d in np.nonzero(ok)[0]] == (list(docs) if want else [])
        assert (np.array(flt.words(), dtype=np.uint32) == words_of(ok)).all() and flt.n_docs == (3 if want else 0), (data, kind, lo, hi)
        flt.close()
    db.close()
    c.close()


# ---- 4. end to end on the corpus of tests/test_gpu_filtered.py ----------------------------------------------------------------------------------

class ListWorld(F.World):
    """F.World plus slot 3's recipe of the reference's test index (oracle/ref_build/ref_driver.cc build_values): per document the ascending,
    duplicate-free set of its slot-0 .. slot-2 values, as ordinals among the distinct ELEMENTS; attached as the list column of slot 0 and of slot 5
    (slot 0 also keeps its plain column: the two must not interfere)."""

    def __init__(self, tmp):
        super().__init__(tmp)
        self.elements = sorted(set(v for s in range(3) for v in self.values[s]))
        rank = {e: i + 1 for i, e in enumerate(self.elements)}
        of = {s: np.array([0] + [rank[v] for v in self.values[s]], dtype=np.uint32) for s in range(3)}
        per_slot = np.stack([of[s][self.ords[s]] for s in range(3)])
        self.lists = [sorted(set(int(x) for x in per_slot[:, d] if x)) for d in range(self.last + 1)]
        self.lists[0] = []
        self.off, self.elem = csr(self.lists)

    def database(self, path, stripe_bits=0):
        db = super().database(path, stripe_bits)
        for slot in (0, 5):
            db.attach_list_column_arrays(slot, self.off, self.elem, len(self.elements))
        return db

    def passes(self, ranges):
        return expected(self.last, ranges, self.ords, {0: self.lists, 5: self.lists})

    def ord_range(self, begin, end):
        import bisect
        return bisect.bisect_left(self.elements, begin) + 1, (ORD_MAX if end is None else bisect.bisect_right(self.elements, end))


@pytest.fixture(scope="module")
def world(built, tmp_path_factory):
    w = ListWorld(str(tmp_path_factory.mktemp("listfilter")))
    yield w
    w.c.close()


def list_filters(w):
    cats = w.values[0]
    return [[(5,) + w.ord_range(cats[3], cats[len(cats) // 2]) + (LIST,)],                           # an interval of categories
            [(0,) + w.ord_range(b"400000", b"700000") + (LIST,)],                                    # a numeric interval
            [(5,) + w.ord_range(cats[10], None)[:1] + (0, GE)],                                      # back() is the category, where there is one
            [(0, 1) + w.ord_range(b"", b"250000")[1:] + (LE,)],                                      # front() is the digit or the number, whichever is smaller
            [(5,) + w.ord_range(b"1", b"3") + (LIST,), (0,) + w.ord_range(cats[5], None)[:1] + (0, GE)],
            [(0,) + w.ord_range(b"100000", b"800000") + (LIST,), (1,) + F.column_ord_range(w.paths[1], b"300000", b"900000")],    # list and plain mixed
            [(0,) + w.ord_range(cats[-1], cats[0]) + (LIST,)]]                                       # begin > end: nothing passes


def test_filtered_searches_under_list_clauses_vs_oracle(world, tmp_path):
    w = world
    db = w.database(str(tmp_path / "s.seg"))
    assert max(len(l) for l in w.lists) == 3 and min(len(l) for l in w.lists[1:]) == 2
    n = (lambda full, quick: quick if QUICK else full)
    queries = (H.gen_term_queries("OR", n(4, 2), 3, 1, 400, maxitems=10, seed=61) + H.gen_term_queries("AND", n(4, 2), 2, 1, 60, maxitems=10, seed=62) +
               H.gen_term_queries("OR", 1, 5, 1, 3000, first=7, maxitems=93, seed=63))
    rng = random.Random(8)
    settings = [(None, 0, False) if qi % 2 == 0 else (rng.choice(["V", "VR", "RV"]), rng.randrange(3), rng.random() < 0.5) for qi in range(len(queries))]
    filters = list_filters(w)
    n_partial = n_items = 0
    for fi, ranges in enumerate(filters):
        flt = db.build_filter(ranges)
        ok = w.passes(ranges)
        assert flt.n_docs == int(ok.sum()), ranges
        assert (flt.n_docs == 0) == (fi == len(filters) - 1), (ranges, flt.n_docs)
        for qi, q in enumerate(queries):
            if (qi + fi) % 2 and not QUICK:
                continue
            mode, slot, rev = settings[qi]                               # (one per query: the oracle ranks each once, whatever the filter)
            spy = (2, len(w.values[2])) if qi % 3 == 0 else None
            got, hdr, counts = search_filtered(db, w.plan(db, q), flt, F.MODES[mode], slot, rev, spy=spy)
            nf, nu = F.check_against_oracle(w, q, mode, slot, rev, ranges, got, hdr, counts, spy[0] if spy else None)
            n_partial += 0 < nf < nu
            n_items += len(got)
        flt.close()
    assert n_partial >= 6 and n_items > 50
    db.close()


def test_search_range_under_list_clauses(world, tmp_path):
    """The filter as the whole query: docid order, and value order with a spy — the first k of the passing documents under (value, docid), the spy's
    counts those of every passing document."""
    w = world
    db = w.database(str(tmp_path / "r.seg"))
    V = _lib.XGM_SORT_VALUE
    for ranges in list_filters(w)[:6]:
        ok = w.passes(ranges)
        flt = db.build_filter(ranges)
        assert 0 < flt.n_docs == int(ok.sum()) < w.last
        docs = np.nonzero(ok)[0]
        got, hdr, _ = search_range(db, flt, 50)
        assert [d for d, _, _, _ in got] == [int(d) for d in docs[:50]] and hdr.matches_exact == len(docs)
        for slot, rev in ((1, False), (0, True)):
            o = w.ords[slot][docs]
            order = np.argsort(~o if rev else o, kind="stable")[:40]
            got, hdr, counts = search_range(db, flt, 40, V, slot, rev, spy=(2, len(w.values[2])))
            assert [(d, x) for d, _, _, x in got] == [(int(docs[i]), int(o[i])) for i in order], (ranges, slot, rev)
            assert counts == np.bincount(w.ords[2][ok], minlength=len(w.values[2]) + 1).tolist() and sum(counts) == hdr.matches_exact == len(docs)
        flt.close()
    db.close()


def test_unfiltered_and_plain_filtered_searches_do_not_move(world, tmp_path):
    """Attaching list columns (one on a slot that has a plain column) and building list filters changes neither an unfiltered search nor a filter of
    XGM_RANGE_VALUE clauses: both still answer as the oracle does, and as they did before any list column was attached."""
    w = world
    db = F.World.database(w, str(tmp_path / "n.seg"), stripe_bits=10)               # plain columns only
    qs = H.gen_term_queries("OR", 3, 3, 1, 400, maxitems=10, seed=251) + H.gen_term_queries("AND", 3, 2, 1, 60, maxitems=10, seed=252)
    plans = [w.plan(db, q) for q in qs]
    plain = [(1,) + F.column_ord_range(w.paths[1], b"150000", b"800000"), (0,) + F.column_ord_range(w.paths[0], w.values[0][4], None)]
    hf = lambda h: (h.n_hits, h.matches_exact, F.wbits(h.max_attained), h.max_weight_subqs_matched, F.wbits(h.max_possible))

    def snapshot():
        flt = db.build_filter(plain)
        out = [flt.words(), flt.n_docs]
        for p in plans:
            got, hdr = search_sorted(db, p, F.MODES["VR"], 0, False)
            fgot, fhdr, counts = search_filtered(db, p, flt, F.MODES["V"], 0, True, spy=(2, len(w.values[2])))
            out.append((got, hf(hdr), fgot, hf(fhdr), counts))
        flt.close()
        return out
    before = snapshot()
    for slot in (0, 5):
        db.attach_list_column_arrays(slot, w.off, w.elem, len(w.elements))
    lf = db.build_filter(list_filters(w)[0])
    search_filtered(db, plans[0], lf)
    lf.close()
    assert snapshot() == before
    flt = db.build_filter(plain)
    assert flt.n_docs == int(F.World.passes(w, plain).sum())
    for q, p in zip(qs, plans):
        got, hdr, _ = search_filtered(db, p, flt, F.MODES["VR"], 1, False)
        F.check_against_oracle(w, q, "VR", 1, False, plain, got, hdr)
        got, hdr = search_sorted(db, p, F.MODES["V"], 2, True)
        full = w.full(q, "V", 2, True)[:q["first"] + q["maxitems"]]
        assert [(d, F.wbits(x), m) for d, x, m, _ in got] == [(d, F.wbits(x), m) for d, x, m, _ in full] and hdr.matches_exact == len(w.full(q, "V", 2, True))
    flt.close()
    db.close()


# ---- 5. the error table -----------------------------------------------------------------------------------------------------------------------------

def test_list_filter_argument_errors(built, tmp_path):
    lastdocid = 40
    c, db = manual_db(tmp_path, lastdocid, "e.seg")
    L = _lib.lib()
    ls = [[]] + [[1 + d % 4] * (d % 3) for d in range(1, lastdocid + 1)]
    off, elem = csr(ls)
    attach_plain(db, 0, np.arange(41, dtype=np.uint32) % 5, 4)
    attach_plain(db, 1, np.arange(41, dtype=np.uint32) % 5, 4)
    db.attach_list_column_arrays(0, off, elem, 4)
    # a bad kind
    for bad in ([(0, 1, 2, 4)], [(0, 1, 2, LIST), (0, 1, 2, 0xFFFFFFFF)], [(0, 0, 2, LIST)], [(0, 0, 2, LE)]):
        with pytest.raises(_lib.XgmError) as e:
            db.build_filter(bad)
        assert e.value.code == _lib.XGM_E_INVALID, bad
    # a list kind on a slot without a LIST column, with or without a plain one
    for kind in (LIST, GE, LE):
        for slot in (1, 6):
            with pytest.raises(_lib.XgmUnsupported):
                db.build_filter([(0, 1, 2, LIST), (slot, 1, 2, kind)])
    c2, db2 = manual_db(tmp_path, lastdocid, "e2.seg")                 # and a plain kind needs the plain column: a list column does not stand in
    db2.attach_list_column_arrays(0, off, elem, 4)
    with pytest.raises(_lib.XgmUnsupported):
        db2.build_filter([(0, 1, 2)])
    db2.close()
    c2.close()
    # bad CSR arrays
    p = lambda a: np.ascontiguousarray(a, dtype=np.uint32).ctypes.data_as(U32)
    call = lambda o, e, n_off=None, n_elem=None, nd=4: L.xgm_index_attach_list_column_ordinals(db._h, 2, p(o), len(o) if n_off is None else n_off, p(e) if len(e) else None,
                                                                                                len(e) if n_elem is None else n_elem, nd)
    assert call(off, elem) == 0
    assert call(off[:-1], elem) == _lib.XGM_E_INVALID                  # n_off != lastdocid + 2
    assert call(off, elem, n_off=1) == _lib.XGM_E_INVALID
    swapped = off.copy()
    swapped[10], swapped[11] = off[11] + 1, off[10]
    assert call(swapped, elem) == _lib.XGM_E_INVALID                   # not monotone
    assert call(off, elem[:-1]) == _lib.XGM_E_INVALID                  # off[n_off - 1] != n_elem
    shifted = off.copy()
    shifted[1] = 1
    assert call(shifted, elem) == _lib.XGM_E_INVALID                   # elements for docid 0
    for v in (0, 5):
        e2 = elem.copy()
        e2[3] = v
        assert call(off, e2) == _lib.XGM_E_INVALID, v                  # an element outside 1 .. n_distinct
    assert L.xgm_index_attach_list_column_ordinals(db._h, 2, None, 42, p(elem), len(elem), 4) == _lib.XGM_E_INVALID
    assert L.xgm_index_attach_list_column_ordinals(None, 2, p(off), 42, p(elem), len(elem), 4) == _lib.XGM_E_INVALID
    assert call(np.zeros(42, dtype=np.uint32), np.zeros(0, dtype=np.uint32)) == 0            # no elements at all: a column nothing passes
    f = db.build_filter([(2, 1, ORD_MAX, LIST)])
    assert f.n_docs == 0 and not any(f.words())
    f.close()
    # n_distinct too large: bit 31 of a head marks a list
    assert call(off, elem, nd=0x7FFFFFFF) == 0
    assert call(off, elem, nd=0x80000000) == _lib.XGM_UNSUPPORTED
    assert call(off, elem, nd=0xFFFFFFFF) == _lib.XGM_UNSUPPORTED
    # a missing or foreign file
    assert L.xgm_index_attach_list_column(db._h, str(tmp_path / "missing").encode()) == _lib.XGM_E_IO
    junk = tmp_path / "junk"
    junk.write_bytes(b"XGMCOL1\0" + bytes(64))
    assert L.xgm_index_attach_list_column(db._h, str(junk).encode()) == _lib.XGM_E_INVALID
    # the working filter still works after all that
    ok = expected(lastdocid, [(0, 2, 3, LIST)], {}, {0: ls})
    check_bitmap(db, [(0, 2, 3, LIST)], ok, "after errors")
    # no device
    nodev = Database(str(tmp_path / "e.seg"), device=_lib.XGM_DEVICE_NONE)
    assert L.xgm_index_attach_list_column_ordinals(nodev._h, 0, p(off), len(off), p(elem), len(elem), 4) == _lib.XGM_E_NO_DEVICE
    assert L.xgm_index_attach_list_column(nodev._h, str(junk).encode()) == _lib.XGM_E_NO_DEVICE
    with pytest.raises(_lib.XgmError) as e:
        nodev.build_filter([(0, 1, 2, LIST)])
    assert e.value.code == _lib.XGM_E_NO_DEVICE
    nodev.close()
    db.close()
    c.close()


def test_list_column_file_attaches_like_the_arrays(built, tmp_path):
    """xgm_index_attach_list_column on a file of the documented layout == attach_list_column_arrays of the same CSR; another lastdocid is refused."""
    import struct
    lastdocid = 300
    c, db = manual_db(tmp_path, lastdocid, "f.seg")
    rng = np.random.RandomState(11)
    ls = [[]] + [[int(x) for x in rng.randint(1, 7, size=rng.randint(0, 4))] for _ in range(lastdocid)]
    off, elem = csr(ls)
    distinct = [b"v%d" % i for i in range(6)]
    voff = np.cumsum([0] + [len(v) for v in distinct]).astype("<u8")
    def write(path, last, off):
        with open(path, "wb") as f:
            f.write(b"XGMLST1\0" + struct.pack("<4IQ", 4, last, 6, 0, len(elem)) + off.astype("<u4").tobytes() + elem.astype("<u4").tobytes() + voff.tobytes() + b"".join(distinct))
        return path
    db.attach_list_column(write(str(tmp_path / "l.col"), lastdocid, off))
    db.attach_list_column_arrays(9, off, elem, 6)
    for kind, lo, hi in ((LIST, 2, 4), (GE, 5, 0), (LE, 1, 2)):
        a, b = db.build_filter([(4, lo, hi, kind)]), db.build_filter([(9, lo, hi, kind)])
        assert a.words() == b.words() == words_of(expected(lastdocid, [(4, lo, hi, kind)], {}, {4: ls})).tolist() and a.n_docs == b.n_docs > 0
        a.close()
        b.close()
    with pytest.raises(_lib.XgmError) as e:
        db.attach_list_column(write(str(tmp_path / "l2.col"), lastdocid + 1, np.append(off, off[-1])))
    assert e.value.code == _lib.XGM_E_INVALID
    db.close()
    c.close()
