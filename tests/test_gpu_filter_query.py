"""Filters from term queries and the filter algebra (include/xgm.h: xgm_filter_build_query, xgm_filter_combine): the bitmap of
xgm_filter_mark_query_kernel word for word against Python set algebra over postings the test writes itself — at the sizes where the word (32), the
bitmap tile (2048), the narrowest and the widest stripe (256, 8192) and the kernel's unit (8192) end, for every stripe width the tests of the format
use, from each of the three membership sources (containers, flat arrays, blocks) —, against the independent device path (xgm_search_all lists the
same documents), xgm_filter_combine_kernel against numpy, and the consumers of a filter (xgm_search_range, xgm_filter_count_pairs,
xgm_search_filtered) on the new filters against numpy and the pinned oracle.

The same file runs under the CPU emulation of the kernels with guard pages behind every device buffer (tests/test_emu_filter_query.py)."""
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
import test_gpu_list_filter as LF
from test_gpu_list_filter import inside
from xapiand_amd import Database, Query, _lib
from xapiand_amd.enquire import (count_pairs, filter_and, filter_and_not, filter_or, plan, search_all, search_filtered, search_range)

pytestmark = [pytest.mark.gpu]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = F.QUICK
AND, OR, AND_NOT = _lib.XGM_FILTER_AND, _lib.XGM_FILTER_OR, _lib.XGM_FILTER_AND_NOT
SWITCHES = ("XGM_NO_DENSE", "XGM_NO_FLAT", "XGM_NO_DENSE XGM_NO_FLAT")
LASTDOCIDS = [1, 31, 32, 33, 255, 256, 257, 2047, 2048, 2049, 8191, 8192, 8193, 16390]
STRIPE_BITS = [0, 10, 8]


def bools_of(flt, lastdocid):
    """The filter's bitmap as one bool per docid 0 .. lastdocid, after the checks every filter owes: the word count, bit 0, the bits beyond lastdocid."""
    w = np.array(flt.words(), dtype=np.uint32)
    assert len(w) == (lastdocid + 32) // 32
    bits = np.unpackbits(w.view(np.uint8), bitorder="little").astype(bool)
    assert not bits[0] and not bits[lastdocid + 1:].any()
    assert flt.n_docs == int(bits.sum())
    return bits[:lastdocid + 1]


def eval_tree(t, sets, n):
    """The documents a tree of helpers.tree_program's form matches, by set algebra: a bool per docid."""
    if isinstance(t, str) or (len(t) == 2 and isinstance(t[1], int) and t[0] not in H.T_KIND):
        return sets.get(t if isinstance(t, str) else t[0], np.zeros(n, dtype=bool))
    op = t[0]
    if op == "SCALE":
        return eval_tree(t[2], sets, n)
    kids = [eval_tree(k, sets, n) for k in t[1:]]
    if op in ("AND", "FILTER"):
        return np.logical_and.reduce(kids)
    if op in ("OR", "SYN"):
        return np.logical_or.reduce(kids)
    if op == "AND_NOT":
        return kids[0] & ~np.logical_or.reduce(kids[1:])
    assert op == "AND_MAYBE"
    return kids[0]


def eval_flat(q, sets, n):
    ts = [sets.get(t, np.zeros(n, dtype=bool)) for t in q["terms"]]
    op, nr = q["op"], q.get("n_required", 0)
    if op == "OR":
        return np.logical_or.reduce(ts)
    if op in ("AND", "PHRASE", "FILTER"):
        return np.logical_and.reduce(ts)
    left = np.logical_and.reduce(ts[:nr])
    return left & ~np.logical_or.reduce(ts[nr:]) if op == "AND_NOT" else left


# ---- 1. the bitmap, word for word ------------------------------------------------------------------------------------------------------

def manual_sets(lastdocid, stripe_bits, wdf255=False):
    """third: every third document (containers from two stripes up); rare: ~1 % (a flat array); edge: the first and the last docid of every stripe and
    lastdocid; bool: wdf 0 postings on ~30 %; `absent` is not in the corpus.  wdf255: one posting of 255 — the library then takes every frequent term's wdf
    bound for 255 (tests/test_gpu_format_edges.py), no such term has a container or a flat array, and the kernel reads BLOCKS in the default configuration."""
    n = lastdocid + 1
    rng = np.random.RandomState(4000 + lastdocid)
    w = 1 << (stripe_bits or 13)
    sets = {k: np.zeros(n, dtype=bool) for k in ("third", "rare", "edge", "bool")}
    sets["third"][1::3] = True
    sets["rare"][rng.rand(n) < 0.01] = True
    sets["rare"][max(1, lastdocid // 2)] = True
    for s in range(lastdocid // w + 1):
        sets["edge"][max(1, s * w)] = sets["edge"][min(lastdocid, (s + 1) * w - 1)] = True
    sets["edge"][lastdocid] = True
    sets["bool"][rng.rand(n) < 0.3] = True
    sets["bool"][lastdocid] = True
    for s in sets.values():
        s[0] = False
    post = {k: [(int(d), 0 if k == "bool" else 1 + int(d) % 3) for d in np.nonzero(v)[0]] for k, v in sets.items()}
    if wdf255:
        post["third"][0] = (post["third"][0][0], 255)
        post["third"][-1] = (post["third"][-1][0], 255)
    return sets, post


FLAT_PLANS = ([dict(op="OR", terms=[t]) for t in ("third", "rare", "edge", "bool", "absent")] +
              [dict(op="AND", terms=["third", "bool"]), dict(op="AND", terms=["bool", "third", "edge"]), dict(op="OR", terms=["rare", "edge"]),
               dict(op="OR", terms=["third", "rare", "edge", "bool", "absent"]), dict(op="AND_NOT", terms=["third", "rare", "bool"], n_required=1),
               dict(op="AND_NOT", terms=["bool", "edge", "third"], n_required=2), dict(op="AND_MAYBE", terms=["third", "edge", "rare"], n_required=2),
               dict(op="AND_MAYBE", terms=["bool", "absent"], n_required=1), dict(op="FILTER", terms=["third", "bool"], n_required=1),
               dict(op="PHRASE", terms=["third", "bool"]), dict(op="AND", terms=["third", "absent"])])
TREES = [("AND", ("OR", "rare", "edge"), "third"),                                   # an OR under an AND
         ("AND_NOT", "third", ("OR", "rare", "bool")),                               # an AND_NOT whose right side is an OR
         ("AND", ("SYN", "rare", "edge", "bool"), "third"),                          # a synonym group
         ("AND", "third", "absent"), ("OR", "third", "absent"),                      # the empty set; its neutral element
         ("AND_NOT", ("OR", "rare", "edge"), ("AND", "third", "bool")),              # two inner nodes meet: both operands on the stack
         ("AND_NOT", "third", ("AND", ("OR", "rare", "edge"), ("OR", "bool", "absent"))),    # the right side is the deeper one: evaluated first
         ("AND_MAYBE", ("OR", "edge", "rare"), ("AND", "third", "bool")),            # the left side's set
         ("OR", ("AND_NOT", "bool", "third"), ("AND_MAYBE", "rare", ("SCALE", 2.0, "edge")))]


def check_manual(tmp_path, lastdocid, stripe_bits, wdf255=False):
    sets, post = manual_sets(lastdocid, stripe_bits, wdf255)
    c = H.ManualCorpus(post, {d: 600 + d % 7 for d in range(1, lastdocid + 1)}, positions=False)
    db = Database(c.build_segment(str(tmp_path / "q.seg"), stripe_bits=stripe_bits))
    assert db.get_lastdocid() == lastdocid
    n, some = lastdocid + 1, 0
    for q in FLAT_PLANS:
        query = Query(q["terms"][0]) if len(q["terms"]) == 1 else Query(q["op"], q["terms"], n_required=q.get("n_required", 0))
        p = plan(db, query, 0, 10)
        assert not (q["op"] == "PHRASE" and p.phrase_active)                 # a corpus without positions: the phrase is planned as its AND
        flt = db.build_query_filter(p)
        want = eval_flat(q, sets, n)
        got = bools_of(flt, lastdocid)
        assert (got == want).all(), (lastdocid, stripe_bits, q, np.nonzero(got != want)[0][:8])
        some += flt.n_docs
        flt.close()
    for tree in TREES:
        flt = db.build_query_filter(plan(db, Query.tree(tree), 0, 10))
        want = eval_tree(tree, sets, n)
        got = bools_of(flt, lastdocid)
        assert (got == want).all(), (lastdocid, stripe_bits, tree, np.nonzero(got != want)[0][:8])
        some += flt.n_docs
        flt.close()
    assert some > 0
    db.close()
    c.close()


@pytest.mark.parametrize("stripe_bits", STRIPE_BITS)
@pytest.mark.parametrize("lastdocid", LASTDOCIDS)
def test_bitmap_equals_set_algebra(built, tmp_path, lastdocid, stripe_bits):
    check_manual(tmp_path, lastdocid, stripe_bits)


@pytest.mark.parametrize("stripe_bits", [0, 8])
@pytest.mark.parametrize("lastdocid", [33, 2049, 8193])
def test_bitmap_from_blocks_in_the_default_configuration(built, tmp_path, lastdocid, stripe_bits):
    """A term whose wdf bound exceeds 254 has neither containers nor a flat array: its membership comes from its blocks, the last of which ends the
    segment's word section."""
    check_manual(tmp_path, lastdocid, stripe_bits, wdf255=True)


# ---- 2. the three membership sources ---------------------------------------------------------------------------------------------------

_first_failure = []


@pytest.mark.parametrize("switch", SWITCHES)
def test_bitmap_with_a_source_switched_off(built, switch):
    """Test 1 once more per A/B switch (read once per process, hence the child): without containers and flat arrays every term is read from its
    blocks, without flat arrays the long-tail terms are."""
    if QUICK:
        pytest.skip("one emulated process per switch is not a quick run")
    assert not _first_failure, "not run: %s" % _first_failure[0]          # one child after the other; after the first that fails none is started
    env = dict(os.environ, **{s: "1" for s in switch.split()})
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                            "-k", "test_bitmap_equals_set_algebra"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        _first_failure.append("%s: killed at its time limit:\n%s" % (switch, (e.stdout or b"")[-2000:]))
        raise AssertionError(_first_failure[0])
    if r.returncode != 0 or "%d passed" % (len(LASTDOCIDS) * len(STRIPE_BITS)) not in r.stdout:
        _first_failure.append("%s failed with %d:\n%s\n%s" % (switch, r.returncode, r.stdout[-3000:], r.stderr[-2000:]))
    assert not _first_failure, _first_failure[0]


# ---- 3. against the independent device path ------------------------------------------------------------------------------------------------

def test_filter_equals_the_documents_search_all_lists(built, tmp_path):
    """Zipf terms over four stripes: ranks up to about 30 have containers, the others flat arrays.  xgm_search_all weighs, lists and orders every match
    through the match kernels; the filter reads membership.  The same docids, the same count."""
    c = H.Corpus(*((2500, 6000) if QUICK else (4000, 10000)))
    db = Database(c.build_segment(str(tmp_path / "a.seg"), stripe_bits=10))
    last = c.v.lastdocid
    n = (lambda full, quick: quick if QUICK else full)
    queries = (H.gen_tree_queries(n(24, 12), 1, 600, seed=91) + H.gen_term_queries("AND", n(4, 2), 2, 1, 60, seed=92) + H.gen_term_queries("AND", n(3, 1), 3, 1, 40, seed=93) +
               H.gen_term_queries("OR", n(3, 1), 2, 1, 2000, seed=94) + H.gen_term_queries("OR", n(3, 1), 5, 1, 3000, seed=95) +
               H.gen_sided_queries("AND_NOT", n(4, 2), 1, 2, 1, 40, 1, 300, seed=96) + H.gen_sided_queries("AND_MAYBE", n(4, 2), 2, 2, 1, 40, 1, 300, seed=97) +
               H.gen_sided_queries("FILTER", n(4, 2), 1, 1, 1, 60, 1, 60, seed=98))
    n_some = 0
    for q in queries:
        p = plan(db, Query.tree(q["tree"]) if "tree" in q else Query(q["op"], q["terms"], n_required=q.get("n_required", 0)), 0, 10)
        rows, hdr = search_all(db, p)
        flt = db.build_query_filter(p)
        got = np.nonzero(bools_of(flt, last))[0].tolist()
        assert got == [d for d, _, _ in rows], q
        assert flt.n_docs == len(rows) == hdr.matches_exact, q
        n_some += 0 < len(rows) < last
        flt.close()
    assert n_some >= len(queries) // 2
    db.close()
    c.close()


# ---- 4 - 6 on the corpus of tests/test_gpu_filtered.py, with the list column of tests/test_gpu_list_filter.py -------------------------------------

class World(LF.ListWorld):
    def docs_of(self, term):
        """One bool per docid: the term's postings as the corpus holds them."""
        if not hasattr(self, "_term_index"):
            self._term_index = {t: i for i, t in enumerate(self.c.terms())}
            self._docs = {}
        if term not in self._docs:
            ok = np.zeros(self.last + 1, dtype=bool)
            ok[self.c.term_postings(self._term_index[term.encode()])[0]] = True
            self._docs[term] = ok
        return self._docs[term]

    def qfilter(self, db, op, terms, n_required=0):
        return db.build_query_filter(plan(db, Query(terms[0]) if len(terms) == 1 else Query(op, terms, n_required=n_required), 0, 10))


@pytest.fixture(scope="module")
def world(built, tmp_path_factory):
    w = World(str(tmp_path_factory.mktemp("filterquery")))
    yield w
    w.c.close()


def plain_ranges(w):
    return ([(1,) + F.column_ord_range(w.paths[1], b"150000", b"600000")], [(0,) + F.column_ord_range(w.paths[0], w.values[0][4], None)],
            [(2, 2, 5), (1,) + F.column_ord_range(w.paths[1], b"300000", b"900000")])


def np_combine(op, a, b):
    return a & b if op == AND else a | b if op == OR else a & ~b


def test_combine_equals_numpy(world, tmp_path):
    w = world
    db = w.database(str(tmp_path / "c.seg"))
    ra, rb, _ = plain_ranges(w)
    made = [(w.qfilter(db, "OR", ["t3", "t40"]), w.docs_of("t3") | w.docs_of("t40")), (w.qfilter(db, "AND", ["t2", "t9"]), w.docs_of("t2") & w.docs_of("t9")),
            (db.build_filter(ra), w.passes(ra)), (db.build_filter(rb), w.passes(rb))]
    before = [f.words() for f, _ in made]
    for f, ok in made:
        assert (bools_of(f, w.last) == ok).all() and 0 < f.n_docs < w.last
    n_partial = 0
    for i, j in ((0, 2), (2, 0), (2, 3), (0, 1), (1, 3), (0, 0), (2, 2)):                # (query, range) both ways, (range, range), (query, query), a == b
        for op, fn in ((AND, filter_and), (OR, filter_or), (AND_NOT, filter_and_not)):
            out = fn(db, made[i][0], made[j][0])
            want = np_combine(op, made[i][1], made[j][1])
            assert (bools_of(out, w.last) == want).all() and out.n_docs == int(want.sum()), (i, j, op)
            assert (out.n_docs == 0) == (i == j and op == AND_NOT), (i, j, op)
            n_partial += 0 < out.n_docs < min(made[i][0].n_docs, made[j][0].n_docs) or op == OR
            out.close()
    assert n_partial >= 12
    assert [f.words() for f, _ in made] == before                                       # the inputs stay as they were
    # the error table
    l = _lib.lib()
    h = C.c_void_p()
    a, b = made[0][0], made[2][0]
    for op in (0, 4, 0xFFFFFFFF):
        assert l.xgm_filter_combine(db._h, op, a._h, b._h, C.byref(h), None) == _lib.XGM_E_INVALID and not h.value
    for args in ((None, AND, a._h, b._h, C.byref(h)), (db._h, AND, None, b._h, C.byref(h)), (db._h, AND, a._h, None, C.byref(h)), (db._h, AND, a._h, b._h, None)):
        assert l.xgm_filter_combine(*args, None) == _lib.XGM_E_INVALID
    c2 = H.ManualCorpus({"a": [(1, 1), (50, 1)]}, {d: 6 for d in range(1, 51)}, positions=False)
    db2 = Database(c2.build_segment(str(tmp_path / "c2.seg")))
    other = db2.build_query_filter(plan(db2, Query("a"), 0, 10))
    assert other.n_docs == 2
    for x, y in ((a, other), (other, a), (other, other)):                               # a filter of another lastdocid, on either side
        assert l.xgm_filter_combine(db._h, AND, x._h, y._h, C.byref(h), None) == _lib.XGM_E_INVALID and not h.value
    nd = C.c_uint64()
    assert l.xgm_filter_combine(db2._h, OR, other._h, other._h, C.byref(h), C.byref(nd)) == 0 and nd.value == 2          # ... and its own index takes it
    l.xgm_filter_free(h)
    nodev = Database(str(tmp_path / "c.seg"), device=_lib.XGM_DEVICE_NONE)
    assert l.xgm_filter_combine(nodev._h, AND, a._h, b._h, C.byref(h), None) == _lib.XGM_E_NO_DEVICE
    nodev.close()
    other.close()
    db2.close()
    c2.close()
    for f, _ in made:
        f.close()
    db.close()


def test_search_range_over_a_term_and_a_range(world, tmp_path):
    """5 (a): no text part — a term as a restriction AND a plain range, paged in docid order and under a value sort with a spy: numpy's stable sort of the
    passing docids (tests/test_gpu_range.py's comparison), every weight +0.0."""
    w = world
    db = w.database(str(tmp_path / "r.seg"))
    V = _lib.XGM_SORT_VALUE
    ranges = plain_ranges(w)[0]
    tf, rf = w.qfilter(db, "OR", ["t5"]), db.build_filter(ranges)
    flt = filter_and(db, tf, rf)
    ok = w.docs_of("t5") & w.passes(ranges)
    docs = np.nonzero(ok)[0]
    assert 50 < len(docs) == flt.n_docs < min(tf.n_docs, rf.n_docs)
    got, hdr, _ = search_range(db, flt, 50)
    assert [d for d, _, _, _ in got] == [int(d) for d in docs[:50]] and hdr.matches_exact == len(docs)
    assert all(F.wbits(x) == 0 and m == 0 for _, x, m, _ in got)
    for slot, rev in ((1, False), (0, True), (2, False)):
        o = w.ords[slot][docs]
        order = np.argsort(~o if rev else o, kind="stable")[:40]
        got, hdr, counts = search_range(db, flt, 40, V, slot, rev, spy=(2, len(w.values[2])))
        assert [(d, x) for d, _, _, x in got] == [(int(docs[i]), int(o[i])) for i in order], (slot, rev)
        assert all(F.wbits(x) == 0 for _, x, _, _ in got)
        assert counts == np.bincount(w.ords[2][ok], minlength=len(w.values[2]) + 1).tolist() and sum(counts) == hdr.matches_exact == len(docs)
    for f in (tf, rf, flt):
        f.close()
    db.close()


def test_reference_range_shape_as_the_whole_query(world, tmp_path):
    """5 (b): OP_FILTER(MultipleValueRange, OR of accuracy terms) — a XGM_RANGE_LIST clause filter AND the query filter of an OR of three terms: the docid
    page is insideRange() restated (tests/test_gpu_list_filter.py: inside) intersected with the union of the terms' postings."""
    w = world
    db = w.database(str(tmp_path / "m.seg"))
    lo, hi = w.ord_range(b"400000", b"700000")
    clause = [(0, lo, hi, LF.LIST)]
    accuracy = ["t4", "t11", "t70"]
    cf, qf = db.build_filter(clause), w.qfilter(db, "OR", accuracy)
    flt = filter_and(db, cf, qf)
    ok = np.array([inside(LF.LIST, l, lo, hi) for l in w.lists], dtype=bool) & np.logical_or.reduce([w.docs_of(t) for t in accuracy])
    docs = np.nonzero(ok)[0]
    assert 20 < len(docs) == flt.n_docs < min(cf.n_docs, qf.n_docs)
    got, hdr, _ = search_range(db, flt, 100)
    assert [d for d, _, _, _ in got] == [int(d) for d in docs[:100]] and hdr.matches_exact == len(docs) and all(F.wbits(x) == 0 for _, x, _, _ in got)
    for f in (cf, qf, flt):
        f.close()
    db.close()


def test_pairs_over_a_query_filter(world, tmp_path):
    """5 (c): the pair spy over a text query's match."""
    w = world
    db = w.database(str(tmp_path / "p.seg"))
    for op, terms, ok in (("OR", ["t7", "t60"], w.docs_of("t7") | w.docs_of("t60")), ("AND", ["t1", "t3"], w.docs_of("t1") & w.docs_of("t3"))):
        flt = w.qfilter(db, op, terms)
        for sa, sb in ((0, 2), (2, 1)):
            cnt = collections.Counter((int(w.ords[sa][d]), int(w.ords[sb][d])) for d in np.nonzero(ok)[0])
            assert count_pairs(db, flt, sa, sb) == sorted((a, b, n) for (a, b), n in cnt.items()) and sum(cnt.values()) == flt.n_docs > 0
        flt.close()
    db.close()


def test_filtered_searches_under_combined_filters_vs_oracle(world, tmp_path):
    """5 (d): a weighted AND under (range OR range) and under (range AND_NOT term): the pinned oracle's full ranking with the same documents dropped
    (the argument of tests/test_gpu_filtered.py: dropping documents from a total order leaves the order of the rest; a filter weighs nothing)."""
    w = world
    db = w.database(str(tmp_path / "s.seg"))
    ra, rb, _ = plain_ranges(w)
    fa, fb, ft = db.build_filter(ra), db.build_filter(rb), w.qfilter(db, "OR", ["t6"])
    cases = [(filter_or(db, fa, fb), w.passes(ra) | w.passes(rb)), (filter_and_not(db, fa, ft), w.passes(ra) & ~w.docs_of("t6"))]
    queries = H.gen_term_queries("AND", 2 if QUICK else 4, 2, 1, 60, maxitems=10, seed=121) + H.gen_term_queries("AND", 1, 3, 1, 30, first=3, maxitems=17, seed=122)
    n_partial = 0
    for flt, ok in cases:
        assert flt.n_docs == int(ok.sum())
        for q in queries:
            got, hdr, _ = search_filtered(db, w.plan(db, q), flt)
            full = w.full(q, None, 0, False)
            filtered = [r for r in full if ok[r[0]]]
            prefix = filtered[:q["first"] + q["maxitems"]]
            assert [(d, F.wbits(x), m) for d, x, m, _ in got] == [(d, F.wbits(x), m) for d, x, m, _ in prefix], q
            assert hdr.matches_exact == len(filtered) and hdr.n_hits == len(prefix), q
            n_partial += 0 < len(filtered) < len(full)
        flt.close()
    assert n_partial >= len(queries)
    for f in (fa, fb, ft):
        f.close()
    db.close()


def test_query_filter_errors_and_threads(world, tmp_path):
    w = world
    seg = str(tmp_path / "e.seg")
    db = w.database(seg)
    l = _lib.lib()
    h = C.c_void_p()
    # positional plans that are active (the corpus has positions) are declined; nothing is built
    for q in (Query("PHRASE", ["t1", "t2"]), Query("NEAR", ["t1", "t2", "t3"], window=6)):
        p = plan(db, q, 0, 10)
        assert p.phrase_active
        with pytest.raises(_lib.XgmUnsupported):
            db.build_query_filter(p)
        assert l.xgm_filter_build_query(db._h, C.byref(p), C.byref(h), None) == _lib.XGM_UNSUPPORTED and not h.value
    p = plan(db, Query("OR", ["t3", "t40"]), 0, 10)
    for args in ((None, C.byref(p), C.byref(h)), (db._h, None, C.byref(h)), (db._h, C.byref(p), None)):
        assert l.xgm_filter_build_query(*args, None) == _lib.XGM_E_INVALID
    nodev = Database(seg, device=_lib.XGM_DEVICE_NONE)
    assert l.xgm_filter_build_query(nodev._h, C.byref(plan(nodev, Query("OR", ["t3", "t40"]), 0, 10)), C.byref(h), None) == _lib.XGM_E_NO_DEVICE and not h.value
    nodev.close()
    # 8 threads on one index: each builds a query filter and a range filter, combines them three ways and reads the words
    ranges = plain_ranges(w)[0]
    qok, rok = w.docs_of("t3") | w.docs_of("t40"), w.passes(ranges)
    want = [LF.words_of(x).tolist() for x in (qok, qok & rok, qok | rok, qok & ~rok)]
    got, errors = {}, []

    def work(t):
        try:
            out = []
            for _ in range(2):
                qf, rf = db.build_query_filter(p), db.build_filter(ranges)
                fs = [qf, filter_and(db, qf, rf), filter_or(db, qf, rf), filter_and_not(db, qf, rf)]
                out.append(([f.words() for f in fs], [f.n_docs for f in fs]))
                for f in fs + [rf]:
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
    counts = [int(x.sum()) for x in (qok, qok & rok, qok | rok, qok & ~rok)]
    assert len(got) == 8 and all(words == want and n == counts for t in range(8) for words, n in got[t])
    db.close()
