"""The live set of an index, Query::MatchAll as a filter, the complement and XOR (include/xgm.h: xgm_filter_all, xgm_index_attach_live,
XGM_FILTER_NOT, XGM_FILTER_XOR): the bitmap of xgm_filter_mark_live_kernel word for word against numpy over lengths and postings the test writes itself
— at the sizes of tests/test_gpu_filter_query.py, where the word (32), the wave's round (256), the bitmap tile (2048) and the widest stripe (8192) end,
and with several tiles (16390) —, the exactness rule (a live document of length 0 beside a deleted one: declined until a live set is attached), the two
new operators of xgm_filter_combine_kernel against numpy with the three old ones beside them, and the consumers of a filter over the new filters.

The kernel's grid is capped at 2048 tiles of 2048 documents: its grid-stride loop takes a second trip only beyond 4 194 304 documents, which no quick
test builds; tools/filter_query_time.py compares the rows `all` and `not` with numpy on a 10 M-document index (three trips) before it times them.

The same file runs under the CPU emulation of the kernels with guard pages behind every device buffer (tests/test_emu_filter_all.py)."""
import collections
import ctypes as C
import threading

import numpy as np
import pytest

import helpers as H
import test_gpu_filter_query as FQ
import test_gpu_filtered as F
import test_gpu_list_filter as LF
from test_gpu_filter_query import bools_of, manual_sets
from xapiand_amd import Database, Query, _lib
from xapiand_amd.enquire import (count_pairs, filter_all, filter_and, filter_and_not, filter_not, filter_or, filter_xor, plan, search_filtered,
                                 search_range)

pytestmark = [pytest.mark.gpu]

QUICK = F.QUICK
AND, OR, AND_NOT, NOT, XOR = _lib.XGM_FILTER_AND, _lib.XGM_FILTER_OR, _lib.XGM_FILTER_AND_NOT, _lib.XGM_FILTER_NOT, _lib.XGM_FILTER_XOR
LASTDOCIDS = FQ.LASTDOCIDS
INVALID, UNSUPPORTED, NO_DEVICE = _lib.XGM_E_INVALID, _lib.XGM_UNSUPPORTED, _lib.XGM_E_NO_DEVICE
P32 = C.POINTER(C.c_uint32)


def words_of(ok):
    """One bool per docid 0 .. lastdocid → the words of xgm_filter_read / xgm_index_attach_live."""
    padded = np.zeros((len(ok) + 31) // 32 * 32, dtype=np.uint8)
    padded[:len(ok)] = ok
    return np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32)


def live_info(db):
    out = (C.c_uint64 * 4)()
    _lib.check(_lib.lib().xgm_debug_live_info(db._h, out))
    return list(out)           # state (0 not asked / 1 held / 2 declined), source (1 no gaps / 2 attached / 3 lengths), kernel launches, marks


def gaps_of(lastdocid):
    """The docids corpus (ii) leaves out: the first and the last docid of a word and of a stripe, lastdocid - 1, every 97th — never docid 1 or lastdocid."""
    gone = {31, 32, 63, 64, 255, 256, 2047, 2048, 8191, 8192, lastdocid - 1} | set(range(97, lastdocid, 97))
    return sorted(d for d in gone if 1 < d < lastdocid)


class LiveCorpus(H.ManualCorpus):
    """manual_sets' postings over documents of which `gone` do not exist and `zero` exist with length 0, their only posting a wdf-0 one of `bool`.
    ManualCorpus counts the documents of non-zero length: doccount is raised by the live ones of length 0."""

    def __init__(self, lastdocid, gone=(), zero=(), stripe_bits=0):
        self.sets, post = manual_sets(lastdocid, stripe_bits)
        gone, zero = set(gone), set(zero)
        assert not gone & zero
        self.live = np.ones(lastdocid + 1, dtype=bool)
        self.live[0] = False
        self.live[sorted(gone)] = False
        for k in self.sets:
            if k != "bool":
                self.sets[k][sorted(gone | zero)] = False
        self.sets["bool"][sorted(gone)] = False
        self.sets["bool"][sorted(zero)] = True
        post = {k: [(int(d), 0 if k == "bool" else 1 + int(d) % 3) for d in np.nonzero(v)[0]] for k, v in self.sets.items() if v.any()}    # (a set left empty: an absent term)
        doclen = {d: 0 if (d in gone or d in zero) else 600 + d % 7 for d in range(1, lastdocid + 1)}
        super().__init__(post, doclen, positions=False)
        self.v.doccount += len(zero)
        assert self.v.doccount == int(self.live.sum()) and self.v.lastdocid == lastdocid


def corpus_of(kind, lastdocid):
    """(i) no gaps, every 5th document of length 0; (ii) gaps, every live length > 0; (iii) the gaps of (ii) and live documents of length 0."""
    if kind == "i":
        return LiveCorpus(lastdocid, zero=range(1, lastdocid + 1, 5))
    gone = gaps_of(lastdocid)
    if kind == "ii":
        return LiveCorpus(lastdocid, gone=gone)
    zero = [d for d in [1, 33, 257, 2049, 8193, lastdocid] + list(range(50, lastdocid, 41)) if 1 <= d <= lastdocid and d not in gone]
    return LiveCorpus(lastdocid, gone=gone, zero=sorted(set(zero)))


def qfilter(db, term):
    return db.build_query_filter(plan(db, Query(term), 0, 10))


def np_combine(op, a, b, live):
    return a & b if op == AND else a | b if op == OR else a & ~b if op == AND_NOT else a ^ b if op == XOR else live & ~a


# ---- 1. the live set, word for word -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lastdocid", LASTDOCIDS)
def test_no_gaps_every_docid_is_live_whatever_its_length(built, tmp_path, lastdocid):
    c = corpus_of("i", lastdocid)
    db = Database(c.build_segment(str(tmp_path / "i.seg")))
    assert db.get_doccount() == db.get_lastdocid() == lastdocid
    flt = filter_all(db)
    assert (bools_of(flt, lastdocid) == c.live).all() and flt.n_docs == lastdocid and bools_of(flt, lastdocid)[1:].all()
    assert live_info(db)[:3] == [1, 1, 1]
    nb = filter_not(db, b := qfilter(db, "bool"))                       # the documents of length 0 are all in `bool`: none of them in its complement
    assert (bools_of(nb, lastdocid) == (c.live & ~c.sets["bool"])).all()
    for f in (flt, nb, b):
        f.close()
    db.close()
    c.close()


@pytest.mark.parametrize("lastdocid", LASTDOCIDS)
def test_gaps_the_set_derived_from_the_lengths(built, tmp_path, lastdocid):
    c = corpus_of("ii", lastdocid)
    db = Database(c.build_segment(str(tmp_path / "ii.seg")))
    n_gone = len(gaps_of(lastdocid))
    assert db.get_doccount() == lastdocid - n_gone
    flt = filter_all(db)
    assert (bools_of(flt, lastdocid) == c.live).all() and flt.n_docs == db.get_doccount()
    assert live_info(db) == [1, 3 if n_gone else 1, 1, db.get_doccount()]
    again = filter_all(db)                                              # from the cache: the same words, no second launch of the marking kernel
    assert again.words() == flt.words() and live_info(db)[2] == 1
    flt.close()                                                         # each filter owns its copy
    assert (bools_of(again, lastdocid) == c.live).all()
    again.close()
    db.close()
    c.close()


@pytest.mark.parametrize("lastdocid", LASTDOCIDS[1:])        # (lastdocid 1 has no room for a gap beside a live document: it is case (a) or empty)
def test_live_documents_of_length_zero_decline_until_a_live_set_is_attached(built, tmp_path, lastdocid):
    c = corpus_of("iii", lastdocid)
    seg = c.build_segment(str(tmp_path / "iii.seg"))
    db = Database(seg)
    l, h = _lib.lib(), C.c_void_p()
    third = qfilter(db, "third")
    for _ in range(2):                                                  # declined, and declined again from the cached outcome
        assert l.xgm_filter_all(db._h, C.byref(h), None) == UNSUPPORTED and not h.value
        assert b"xgm_index_attach_live" in l.xgm_last_error()
        assert l.xgm_filter_combine(db._h, NOT, third._h, None, C.byref(h), None) == UNSUPPORTED and not h.value
        assert b"xgm_index_attach_live" in l.xgm_last_error()
    with pytest.raises(_lib.XgmUnsupported):
        filter_all(db)
    assert live_info(db)[0] == 2 and live_info(db)[2] == 1
    # what needs no live set still works
    rare, boo = qfilter(db, "rare"), qfilter(db, "bool")
    assert (bools_of(boo, lastdocid) == c.sets["bool"]).all()
    for op, fn in ((AND, filter_and), (OR, filter_or), (AND_NOT, filter_and_not), (XOR, filter_xor)):
        out = fn(db, third, boo)
        assert (bools_of(out, lastdocid) == np_combine(op, c.sets["third"], c.sets["bool"], None)).all(), op
        out.close()
    db.close()
    # (iv) a fresh index of the same segment with the live set attached: exact, the documents of length 0 included
    db = Database(seg)
    db.attach_live(words_of(c.live))
    assert live_info(db)[:3] == [1, 2, 0]
    flt = filter_all(db)
    assert (bools_of(flt, lastdocid) == c.live).all() and flt.n_docs == db.get_doccount() == int(c.live.sum())
    b2 = qfilter(db, "bool")
    nb = filter_not(db, b2)
    assert (bools_of(nb, lastdocid) == (c.live & ~c.sets["bool"])).all()
    assert live_info(db)[2] == 0                                        # the lengths were never consulted
    for f in (third, rare, boo, flt, b2, nb):
        f.close()
    db.close()
    # ... and an attach AFTER a decline is taken too: nothing had been handed out
    db = Database(seg)
    assert l.xgm_filter_all(db._h, C.byref(h), None) == UNSUPPORTED
    db.attach_live(words_of(c.live))
    flt = filter_all(db)
    assert (bools_of(flt, lastdocid) == c.live).all()
    flt.close()
    db.close()
    c.close()


# ---- 2. the attach error table ---------------------------------------------------------------------------------------------------------------

def attach(db, w):
    w = np.ascontiguousarray(w, dtype=np.uint32)
    return _lib.lib().xgm_index_attach_live(db._h, w.ctypes.data_as(P32), len(w))


def test_attach_errors_and_the_file_form(built, tmp_path):
    last = 300
    c = corpus_of("iii", last)
    seg = c.build_segment(str(tmp_path / "e.seg"))
    good = words_of(c.live)
    l = _lib.lib()
    db = Database(seg)
    assert l.xgm_index_attach_live(None, good.ctypes.data_as(P32), len(good)) == INVALID
    assert l.xgm_index_attach_live(db._h, None, len(good)) == INVALID
    assert attach(db, good[:-1]) == INVALID and attach(db, np.append(good, 0)) == INVALID            # another n_words
    gone = gaps_of(last)[0]
    live_d = int(np.nonzero(c.live)[0][3])
    bad = good.copy(); bad[0] |= 1                                                                      # bit 0
    assert attach(db, bad) == INVALID
    bad[live_d >> 5] &= ~np.uint32(1 << (live_d & 31))                                                  # ... with the popcount kept
    assert attach(db, bad) == INVALID
    bad = good.copy(); bad[-1] |= np.uint32(1 << ((last & 31) + 1)); bad[live_d >> 5] &= ~np.uint32(1 << (live_d & 31))   # a bit beyond lastdocid, the popcount kept
    assert attach(db, bad) == INVALID
    bad = good.copy(); bad[gone >> 5] |= np.uint32(1 << (gone & 31))                                    # popcount one too many
    assert attach(db, bad) == INVALID
    bad = good.copy(); bad[live_d >> 5] &= ~np.uint32(1 << (live_d & 31))                               # ... one too few
    assert attach(db, bad) == INVALID
    assert live_info(db)[0] == 0                                                                        # none of them left anything behind
    assert attach(db, good) == 0
    assert attach(db, good) == INVALID                                                                  # a second attach
    flt = filter_all(db)
    assert (bools_of(flt, last) == c.live).all()
    flt.close()
    db.close()
    nodev = Database(seg, device=_lib.XGM_DEVICE_NONE)
    assert attach(nodev, good) == NO_DEVICE
    assert l.xgm_index_attach_live_file(nodev._h, b"/nonexistent") == NO_DEVICE
    h = C.c_void_p()
    assert l.xgm_filter_all(nodev._h, C.byref(h), None) == NO_DEVICE and not h.value
    nodev.close()
    # an attach after the first use: corpus (ii) builds its set from the lengths, after which it is the index's for good
    c2 = corpus_of("ii", last)
    db2 = Database(c2.build_segment(str(tmp_path / "e2.seg")))
    flt = filter_all(db2)
    assert attach(db2, words_of(c2.live)) == INVALID
    assert l.xgm_filter_all(None, C.byref(h), None) == INVALID and l.xgm_filter_all(db2._h, None, None) == INVALID
    flt.close()
    # the file form: "XGMLIV1\0", lastdocid, doccount, n_words, 0, the words
    path = str(tmp_path / "live.bin")
    hdr = np.array([last, int(c.live.sum()), len(good), 0], dtype=np.uint32)
    open(path, "wb").write(b"XGMLIV1\0" + hdr.tobytes() + good.tobytes())
    db = Database(seg)
    db.attach_live_file(path)
    flt = filter_all(db)
    assert (bools_of(flt, last) == c.live).all() and live_info(db)[:2] == [1, 2]
    flt.close()
    db.close()
    # a file of another lastdocid, a truncated one, another magic
    c3 = corpus_of("iii", last + 1)
    db3 = Database(c3.build_segment(str(tmp_path / "e3.seg")))
    assert l.xgm_index_attach_live_file(db3._h, path.encode()) == INVALID
    assert l.xgm_index_attach_live_file(db3._h, str(tmp_path / "missing").encode()) == _lib.XGM_E_IO
    db = Database(seg)
    open(path + ".short", "wb").write(b"XGMLIV1\0" + hdr.tobytes() + good.tobytes()[:-4])
    open(path + ".magic", "wb").write(b"XGMCOL1\0" + hdr.tobytes() + good.tobytes())
    assert l.xgm_index_attach_live_file(db._h, (path + ".short").encode()) == INVALID
    assert l.xgm_index_attach_live_file(db._h, (path + ".magic").encode()) == INVALID
    assert live_info(db)[0] == 0
    for x in (db, db2, db3):
        x.close()
    for x in (c, c2, c3):
        x.close()


# ---- 3. NOT and XOR against numpy; 4. the error table of combine ---------------------------------------------------------------------------------

@pytest.mark.parametrize("lastdocid", [33, 2049, 16390] if QUICK else [33, 257, 2049, 8193, 16390])
def test_not_and_xor_equal_numpy(built, tmp_path, lastdocid):
    c = corpus_of("ii", lastdocid)
    db = Database(c.build_segment(str(tmp_path / "n.seg")))
    live = c.live
    names = ("third", "rare", "edge", "bool", "absent")
    sets = dict(c.sets, absent=np.zeros(lastdocid + 1, dtype=bool), all=live)
    made = {k: qfilter(db, k) for k in names}
    made["all"] = filter_all(db)
    before = {k: f.words() for k, f in made.items()}
    for k, f in made.items():
        assert (bools_of(f, lastdocid) == sets[k]).all(), k
    for k, f in made.items():
        n = filter_not(db, f)
        got = bools_of(n, lastdocid)
        assert (got == (live & ~sets[k])).all() and not got[gaps_of(lastdocid)].any(), k          # a complement raises no deleted docid
        assert n.n_docs == db.get_doccount() - f.n_docs
        nn = filter_not(db, n)
        assert (bools_of(nn, lastdocid) == sets[k]).all(), k                                       # not(not(a)) == a: the filters hold live documents only
        n.close()
        nn.close()
    n_absent, n_all = filter_not(db, made["absent"]), filter_not(db, made["all"])
    assert n_absent.words() == made["all"].words() and n_absent.n_docs == db.get_doccount()
    assert n_all.n_docs == 0 and not any(n_all.words())
    n_absent.close()
    n_all.close()
    pairs = [("third", "rare"), ("rare", "third"), ("edge", "bool"), ("bool", "third"), ("third", "absent"), ("all", "bool"), ("third", "third")]
    for ka, kb in pairs:
        a, b, sa, sb = made[ka], made[kb], sets[ka], sets[kb]
        outs = {op: a.combine(b, op, db) for op in (AND, OR, AND_NOT, XOR)}
        for op, out in outs.items():                                                                 # the new op beside the three old ones
            want = np_combine(op, sa, sb, live)
            assert (bools_of(out, lastdocid) == want).all() and out.n_docs == int(want.sum()), (ka, kb, op)
        assert (outs[XOR].n_docs == 0) == (ka == kb)                                                 # a ^ a is empty
        both_not = filter_and_not(db, outs[OR], outs[AND])                                           # a ^ b == (a | b) & ~(a & b)
        assert both_not.words() == outs[XOR].words()
        na, nb, nor = filter_not(db, a), filter_not(db, b), filter_not(db, outs[OR])                 # not(a | b) == not(a) & not(b)
        de_morgan = filter_and(db, na, nb)
        assert nor.words() == de_morgan.words() and nor.n_docs == de_morgan.n_docs
        for f in list(outs.values()) + [both_not, na, nb, nor, de_morgan]:
            f.close()
    assert {k: f.words() for k, f in made.items()} == before                                         # the inputs stay as they were
    # the error table
    l, h = _lib.lib(), C.c_void_p()
    a, b = made["third"], made["rare"]
    for op in (0, 6, 0xFFFFFFFF):
        assert l.xgm_filter_combine(db._h, op, a._h, b._h, C.byref(h), None) == INVALID and not h.value
        assert l.xgm_filter_combine(db._h, op, a._h, None, C.byref(h), None) == INVALID and not h.value
    assert l.xgm_filter_combine(db._h, NOT, a._h, b._h, C.byref(h), None) == INVALID and not h.value      # NOT takes one filter
    assert l.xgm_filter_combine(db._h, NOT, a._h, a._h, C.byref(h), None) == INVALID and not h.value
    assert l.xgm_filter_combine(db._h, XOR, a._h, None, C.byref(h), None) == INVALID and not h.value      # XOR takes two
    assert l.xgm_filter_combine(db._h, XOR, None, b._h, C.byref(h), None) == INVALID
    assert l.xgm_filter_combine(db._h, NOT, None, None, C.byref(h), None) == INVALID
    assert l.xgm_filter_combine(db._h, NOT, a._h, None, None, None) == INVALID
    c2 = H.ManualCorpus({"a": [(1, 1), (50, 1)]}, {d: 6 for d in range(1, 51)}, positions=False)
    db2 = Database(c2.build_segment(str(tmp_path / "n2.seg")))
    other = qfilter(db2, "a")
    for x, y in ((a, other), (other, a)):                                                            # a filter of another lastdocid, on either side
        assert l.xgm_filter_combine(db._h, XOR, x._h, y._h, C.byref(h), None) == INVALID and not h.value
    assert l.xgm_filter_combine(db._h, NOT, other._h, None, C.byref(h), None) == INVALID and not h.value
    nd = C.c_uint64()
    assert l.xgm_filter_combine(db2._h, NOT, other._h, None, C.byref(h), C.byref(nd)) == 0 and nd.value == 48   # ... and its own index takes it
    l.xgm_filter_free(h)
    other.close()
    db2.close()
    c2.close()
    for f in made.values():
        f.close()
    db.close()
    c.close()


# ---- 5. consumers over the new filters -------------------------------------------------------------------------------------------------------------

def test_search_range_over_the_all_filter(built, tmp_path):
    """MatchAll as the whole query: the first k live docids, weights +0.0 as bits; under a value sort with a spy the (value, docid) order of the live
    documents — numpy's stable sort, ordinal 0 (no value) first ascending and last under `reverse`, as tests/test_gpu_range.py has it — and the
    column's histogram over the live documents."""
    last = 2500
    c = corpus_of("ii", last)
    db = Database(c.build_segment(str(tmp_path / "r.seg")))
    rng = np.random.RandomState(77)
    ords = {}
    for slot, nd in ((0, 40), (1, 7)):
        o = rng.randint(1, nd + 1, size=last + 1).astype(np.uint32)
        o[rng.rand(last + 1) < 0.15] = 0                                 # documents without a value
        o[gaps_of(last)] = 0                                             # a deleted document has none
        o[0] = 0
        ords[slot] = o
        _lib.check(_lib.lib().xgm_index_attach_column_ordinals(db._h, slot, o.ctypes.data_as(P32), last + 1, nd))
    flt = filter_all(db)
    docs = np.nonzero(c.live)[0]
    dc = db.get_doccount()
    for k in (1, 10, 1000):
        got, hdr, _ = search_range(db, flt, k)
        assert [d for d, _, _, _ in got] == [int(d) for d in docs[:k]]
        assert all(F.wbits(x) == 0 and m == 0 and o == 0 for _, x, m, o in got)
        assert hdr.matches_exact == dc == len(docs) and hdr.n_hits == min(k, dc)
    for slot, rev, nd in ((0, False, 40), (0, True, 40), (1, False, 7)):
        o = ords[slot][docs]
        order = np.argsort(~o if rev else o, kind="stable")[:60]
        got, hdr, counts = search_range(db, flt, 60, _lib.XGM_SORT_VALUE, slot, rev, spy=(1, 7))
        assert [(d, x) for d, _, _, x in got] == [(int(docs[i]), int(o[i])) for i in order], (slot, rev)
        assert all(F.wbits(x) == 0 for _, x, _, _ in got)
        assert counts == np.bincount(ords[1][docs], minlength=8).tolist() and sum(counts) == hdr.matches_exact == dc
        assert counts[0] > 0
    # the pair spy over a complement
    third = qfilter(db, "third")
    nt = filter_not(db, third)
    ok = c.live & ~c.sets["third"]
    cnt = collections.Counter((int(ords[0][d]), int(ords[1][d])) for d in np.nonzero(ok)[0])
    assert count_pairs(db, nt, 0, 1) == sorted((a, b, n) for (a, b), n in cnt.items()) and sum(cnt.values()) == nt.n_docs > 0
    for f in (flt, third, nt):
        f.close()
    db.close()
    c.close()


@pytest.fixture(scope="module")
def world(built, tmp_path_factory):
    w = FQ.World(str(tmp_path_factory.mktemp("filterall")))
    yield w
    w.c.close()


def test_filtered_search_under_a_complement_vs_oracle(world, tmp_path):
    """xgm_search_filtered(q, not f): the pinned oracle's full ranking with the documents of f dropped (tests/test_gpu_filtered.py's argument: dropping
    documents from a total order leaves the order of the rest; a filter weighs nothing)."""
    w = world
    db = w.database(str(tmp_path / "s.seg"))
    ft = w.qfilter(db, "OR", ["t6"])
    flt = filter_not(db, ft)
    ok = ~w.docs_of("t6")
    ok[0] = False
    assert flt.n_docs == int(ok.sum()) == db.get_doccount() - ft.n_docs
    queries = H.gen_term_queries("AND", 2 if QUICK else 4, 2, 1, 60, maxitems=10, seed=131) + H.gen_term_queries("OR", 1, 2, 1, 300, first=3, maxitems=17, seed=132)
    n_partial = 0
    for q in queries:
        got, hdr, _ = search_filtered(db, w.plan(db, q), flt)
        full = w.full(q, None, 0, False)
        filtered = [r for r in full if ok[r[0]]]
        prefix = filtered[:q["first"] + q["maxitems"]]
        assert [(d, F.wbits(x), m) for d, x, m, _ in got] == [(d, F.wbits(x), m) for d, x, m, _ in prefix], q
        assert hdr.matches_exact == len(filtered) and hdr.n_hits == len(prefix), q
        n_partial += 0 < len(filtered) < len(full)
    assert n_partial >= 1
    # 7. the Zipf corpus: all == doccount, not(term) == doccount - termfreq for a frequent, a rare and an absent term
    fa = filter_all(db)
    assert fa.n_docs == db.get_doccount() == w.last and bools_of(fa, w.last)[1:].all()
    terms = w.c.terms()
    rare = terms[len(terms) // 2].decode()                               # by Zipf's law nearly every term is rare
    for term in ("t1", rare, "nosuchterm"):
        tf = db.get_termfreq(term) if term.encode() in terms else 0
        f = w.qfilter(db, "OR", [term])
        n = filter_not(db, f)
        assert f.n_docs == tf and n.n_docs == db.get_doccount() - tf, term
        assert (bools_of(n, w.last)[1:] == ~bools_of(f, w.last)[1:]).all()
        f.close()
        n.close()
    assert db.get_termfreq("t1") > 20 * db.get_termfreq(rare) > 0
    for f in (ft, flt, fa):
        f.close()
    db.close()


# ---- 6. first use from 8 threads ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first", ["all", "not"])
def test_first_use_from_eight_threads_builds_one_set(built, tmp_path, first):
    last = 8193
    c = corpus_of("ii", last)
    db = Database(c.build_segment(str(tmp_path / "t.seg")))
    third = qfilter(db, "third")
    assert live_info(db) == [0, 0, 0, 0]
    want = c.live if first == "all" else c.live & ~c.sets["third"]
    got, errors = {}, []
    gate = threading.Barrier(8)

    def work(t):
        try:
            gate.wait()
            f = filter_all(db) if first == "all" else filter_not(db, third)
            got[t] = (f.words(), f.n_docs)
            f.close()
        except Exception as e:                                           # (an assertion inside a thread would be lost)
            errors.append(repr(e))
    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    ww = words_of(want).tolist()
    assert len(got) == 8 and all(w == ww and n == int(want.sum()) for w, n in got.values())
    assert live_info(db) == [1, 3, 1, db.get_doccount()]                 # one cached set, made by one launch
    third.close()
    db.close()
    c.close()
