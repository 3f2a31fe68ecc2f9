"""Nested queries (XGM_OP_TREE) at the edges of the lowering (xgm_plan.cc::plan_tree) and of the match kernel's node program
(xgm_match_body.inc), and their boolean form (xgm_filter_terms.h): the explicit cases of helpers.tree_edge_cases() on the crafted corpus of
helpers.tree_edge_postings() — tied estimates in every query order, roots that are groups, one-child operators, the flattening rules, sided
operators with several right-hand children, absent terms at every position (a weighted synonym group of absent terms is no postlist at all),
a term in every document, synonym sums at the width of the wdf tables, 16 terms / 40 ops, OP_WILDCARD — against the CPU oracle, which
tests/test_oracle_vs_reference.py and tests/golden/tree_edges.json pin bit for bit to the compiled reference on these very cases.

The same file runs under the CPU emulation of the kernels with guard pages behind every device buffer (tests/test_emu_tree_edges.py)."""
import collections

import numpy as np
import pytest

import helpers as H
from test_batch_plan import plan_dump
from xapiand_amd import Database, Query, _lib, merged_stats, plan, search_batch
from xapiand_amd.enquire import search_all

pytestmark = pytest.mark.gpu

PAGES = [(0, 1), (0, 10), (3, 7), (0, 300)]
STRIPE_BITS = [8, 10]
LAST = H.TREE_EDGE_LASTDOCID
# the cases that match nothing — by construction; every other case matches something (test_the_cases_reach_the_edges)
EMPTY = {"absent_root", "absent_and", "absent_or_all", "absent_syn_all", "absent_andnot_left", "absent_maybe_left", "absent_filter_right",
         "absent_filter_left", "absent_syn_all_filter_right", "all_andnot_right", "all_zero_estimates_tie"}
FLAT = [("AND", ["eqA", "eqB"]), ("AND", ["o20", "o22", "o21"]), ("OR", ["o10", "o11", "one", "o12"]), ("OR", ["w254a", "w255"]),
        ("AND", ["m3", "m1", "m2", "m0"]), ("OR", ["first", "last", "nosuch1"])]


class World:
    def __init__(self, d):
        post, doclen = H.tree_edge_postings()
        self.post, self.doclen = post, doclen
        self.c = H.ManualCorpus(post, doclen)
        self.seg = {sb: self.c.build_segment(str(d / ("e%d.seg" % sb)), stripe_bits=sb) for sb in STRIPE_BITS}
        self.db = {sb: Database(p) for sb, p in self.seg.items()}
        self.cases = H.tree_edge_cases() + H.tree_edge_unpinned_cases()
        self._want = {}
        # the two halves of a batch by the width of the wdf tables a case needs: 2 bytes once a term's wdf bound exceeds 254
        db = self.db[STRIPE_BITS[0]]
        self.is_wide = {n: any(db.get_wdf_upper_bound(t) > 254 for t in H.tree_program(t_)[0]) for n, t_ in self.cases}

    def want(self, name, tree, first, maxitems):
        """The oracle's (rows, hdr, total_subqs): computed once per (case, page), shared by the tests, never changed."""
        key = (name, first, maxitems)
        if key not in self._want:
            self._want[key] = H.oracle_search_tree(self.c, tree, first, maxitems)
        return self._want[key]

    def close(self):
        for db in self.db.values():
            db.close()
        self.c.close()


@pytest.fixture(scope="module")
def world(built, tmp_path_factory):
    w = World(tmp_path_factory.mktemp("tree_edges"))
    yield w
    w.close()


def check(w, name, tree, p, hits, hdr, first, maxitems):
    rows, oh, tot = w.want(name, tree, first, maxitems)
    got = [(h.docid, h.weight, h.subqs_matched) for h in hits]
    assert got == rows, (name, first, maxitems, got[:3], rows[:3])
    assert hdr.matches_exact == oh.matches, (name, hdr.matches_exact, oh.matches)
    assert hdr.max_possible == oh.max_possible, (name, hdr.max_possible, oh.max_possible)
    assert p.total_subqs == tot, (name, p.total_subqs, tot)
    assert (hdr.max_attained, hdr.max_weight_subqs_matched) == (oh.max_attained, oh.max_subqs), (name, hdr.max_attained, oh.max_attained)
    return len(rows)


@pytest.mark.parametrize("stripe_bits", STRIPE_BITS)
def test_pages_vs_oracle(world, stripe_bits):
    """Every case at every page.  The cases whose terms all keep a wdf bound of 254 or less go in batches of their own: launches of the 8-bit
    instantiation — where SYN(w254a, w254b) sums 508 from two bytes — beside launches of the 16-bit one."""
    w, db = world, world.db[stripe_bits]
    n_hits = collections.Counter()
    for first, maxitems in PAGES:
        for wide in (False, True):
            mine = [(n, t) for n, t in w.cases if w.is_wide[n] == wide]
            plans = [plan(db, Query.tree(t), first, maxitems) for _, t in mine]
            for (n, t), p, (hits, hdr) in zip(mine, plans, search_batch(db, plans)):
                n_hits[wide] += check(w, n, t, p, hits, hdr, first, maxitems)
    assert n_hits[False] > 1000 and n_hits[True] > 3000, n_hits


@pytest.mark.parametrize("stripe_bits", STRIPE_BITS)
def test_one_heterogeneous_batch(world, stripe_bits):
    """All the cases in ONE batch, pages mixed, with flat conjunctions and disjunctions: the batch is wide, so the narrow cases are answered
    from the 16-bit tables this time."""
    w, db = world, world.db[stripe_bits]
    pages = [PAGES[i % len(PAGES)] for i in range(len(w.cases))]
    plans = [plan(db, Query.tree(t), f, k) for (_, t), (f, k) in zip(w.cases, pages)]
    fplans = [plan(db, Query(op, terms), 0, 10) for op, terms in FLAT]
    got = search_batch(db, plans + fplans)
    for (n, t), p, (hits, hdr), (f, k) in zip(w.cases, plans, got, pages):
        check(w, n, t, p, hits, hdr, f, k)
    for (op, terms), (hits, hdr) in zip(FLAT, got[len(plans):]):
        want, oh = H.oracle_search(w.c, op, terms, 0, 10)
        assert [(h.docid, h.weight, h.subqs_matched) for h in hits] == want and want, (op, terms)
        assert hdr.matches_exact == oh.matches and hdr.max_possible == oh.max_possible


@pytest.mark.parametrize("stripe_bits", STRIPE_BITS)
def test_whole_match_and_query_filter(world, stripe_bits):
    """xgm_search_all lists every matching document with its weight bits; xgm_filter_build_query marks the same documents from posting membership
    alone.  Both against the oracle's whole match.  The filter's program builder takes every case (16 groups need 5 of its 6 stack values, 16 leaf
    and 15 node operations 31 of its 64 code bytes): a decline would be an accident, and fails here."""
    w, db = world, world.db[stripe_bits]
    declined, n_docs = [], 0
    for n, t in w.cases:
        rows, oh, _ = w.want(n, t, 0, LAST)
        assert oh.matches == len(rows)
        by_docid = sorted(rows)
        p = plan(db, Query.tree(t), 0, 10)
        if rows:
            got, hdr = search_all(db, p)
            assert got == by_docid, (n, got[:3], by_docid[:3])
            assert hdr.matches_exact == len(rows), n
        try:
            flt = db.build_query_filter(p)
        except _lib.XgmUnsupported:
            declined.append(n)
            continue
        words = np.array(flt.words(), dtype=np.uint32)
        assert len(words) == (LAST + 32) // 32
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")
        assert np.nonzero(bits)[0].tolist() == [d for d, _, _ in by_docid], n
        assert flt.n_docs == len(rows), n
        n_docs += flt.n_docs
        flt.close()
    assert declined == []
    assert n_docs > 20000


def test_two_shards_with_merged_statistics(world, tmp_path):
    """Xapiand's per-shard protocol on the crafted corpus cut into two docid-interleaved shards: every shard plans with the merged statistics
    but orders by its own estimates — which differ from shard to shard and from the whole corpus's (the ties fall apart, others appear) — and a
    term one shard lacks (one, first, last, w255's tail) has tf_local == 0 < tf_global there."""
    w = world
    shards = []
    for s in range(2):
        post = {t: [((d - 1) // 2 + 1, wdf, pos) for d, wdf, pos in pl if (d - 1) % 2 == s] for t, pl in w.post.items()}
        shards.append(H.ManualCorpus({t: pl for t, pl in post.items() if pl}, {(d - 1) // 2 + 1: l for d, l in w.doclen.items() if (d - 1) % 2 == s}))
    dbs = [Database(c.build_segment(str(tmp_path / ("s%d.seg" % s)), stripe_bits=8)) for s, c in enumerate(shards)]
    n_lacking = n_hits = 0
    for n, t in w.cases:
        query = Query.tree(t)
        gs = merged_stats(dbs, query)
        terms = [x.decode() for x in query.terms]
        g = dict(total_length=gs.total_length, collection_size=gs.collection_size, termfreq={x: gs.termfreq[i] for i, x in enumerate(terms)})
        plans = [plan(db, query, 0, 20, global_stats=gs) for db in dbs]
        for s, (db, c, p) in enumerate(zip(dbs, shards, plans)):
            n_lacking += any(c.termfreq(x) == 0 < g["termfreq"][x] for x in terms)
            (hits, hdr), = search_batch(db, [p])
            rows, oh, tot = H.oracle_search_tree(c, t, 0, 20, global_stats=g)
            assert [(h.docid, h.weight, h.subqs_matched) for h in hits] == rows, (s, n)
            assert hdr.max_possible == oh.max_possible and hdr.matches_exact == oh.matches and p.total_subqs == tot, (s, n)
            n_hits += len(rows)
    assert n_lacking >= 8 and n_hits > 1500
    for d in dbs:
        d.close()
    for c in shards:
        c.close()


def test_the_cases_reach_the_edges(world):
    """The cases are what they claim to be: both table widths are launched, a root is a group, sixteen groups occur, the ties are ties, the
    wildcards' lists are the corpus's expansions, the empty answers are empty and the others are not."""
    w = world
    host = Database(w.seg[8], device=_lib.XGM_DEVICE_NONE)
    by_name = dict(w.cases)
    narrow = [Query.tree(t) for n, t in w.cases if not w.is_wide[n]]
    wide = [Query.tree(t) for n, t in w.cases if w.is_wide[n]]
    assert len(narrow) >= 20 and len(wide) >= 20
    assert plan_dump(host, narrow)[0]["wide"] == 0 and plan_dump(host, wide)[0]["wide"] == 1 and plan_dump(host, narrow[:3] + wide[:1])[0]["wide"] == 1
    assert not w.is_wide["width_syn_508"] and not w.is_wide["width_syn_508_in_or"] and w.is_wide["width_syn_255"] and w.is_wide["width_syn_808"]
    plans = {n: plan(host, Query.tree(t), 0, 10) for n, t in w.cases}
    roots = [n for n, p in plans.items() if p.tree_len == 0]
    assert {"root_term", "root_term_wqf", "root_scale", "root_scale_scale", "root_syn", "root_syn_of_one", "one_and", "wild_root_eq", "wild_of_one"} <= set(roots)
    assert plans["limit_and16"].n_groups == 16 and plans["limit_or16"].n_groups == 16 and plans["limit_and16"].tree_len == 15
    assert plans["limit_and_syn8"].n_groups == 8 and plans["limit_and_syn8"].n_terms == 16
    assert len(H.tree_program(by_name["limit_prog40"])[2]) == _lib.XGM_MAX_TREE and plans["limit_prog40"].n_groups == 16
    # the ties: equal df; a leaf's df equal to a group's and to an OR's estimate, as the planner computes them
    assert len({host.get_termfreq(t) for t in ("eqA", "eqB", "eqC", "eqD")}) == 1
    assert plan(host, Query.tree(("SYN", "eqS1", "eqS2")), 0, 10).est_est == host.get_termfreq("eqL") == plans["tie_and_syn_leaf"].est_max
    assert plan(host, Query.tree(("OR", "eqA", "eqB")), 0, 10).est_est == host.get_termfreq("eqO")
    assert host.get_termfreq("all") == host.get_doccount() == 2560 and host.get_lastdocid() == LAST
    assert plans["all_andnot_right"].est_est == 0
    assert all(host.get_termfreq(t) == 0 for t in H.TREE_EDGE_ABSENT)
    # the wildcards list what the corpus holds under the prefix, in term order
    names = [t.decode() for t in w.c.terms()]
    for p in ("eq", "m", "w25", "fir", "las"):
        assert H.tree_edge_prefix(p) == sorted(t for t in names if t.startswith(p)) != []
    # a weighted synonym group of absent terms is dropped: the OR's bound is the bound of the others
    assert plans["absent_syn_all_in_or"].max_possible == plan(host, Query.tree(("OR", "eqA", "eqB", "eqC")), 0, 10).max_possible
    assert plans["absent_syn_all"].max_possible == 0.0 and plans["absent_syn_all_in_and_in_or"].total_subqs == 3
    # an AND_MAYBE under a zero factor is its left side: the right side is not lowered — its terms stand in a group no node reads.  (Lowering it
    # would change no answer: an unweighted right side adds +0.0 and counts nothing; the plan is where the rule shows.)
    for name, n_nodes, dropped in (("flat_maybe_zero_in_filter", 1, ["eqC"]), ("flat_maybe_zero_in_andnot", 1, ["eqB"]), ("flat_maybe_zero_deep", 2, ["o03", "o04"])):
        p, terms = plans[name], H.tree_program(by_name[name])[0]
        read = {x for j in range(p.tree_len) for x in (p.tree_a[j], p.tree_b[j]) if x < p.n_groups}
        assert p.tree_len == n_nodes and all(p.group_of[terms.index(t)] not in read for t in dropped), name
        assert len({p.group_of[terms.index(t)] for t in dropped}) == 1 and p.n_groups == len(terms) - len(dropped) + 1, name
    # every edge has its cases; the empty answers are empty, the others are not
    per_edge = collections.Counter(n.split("_")[0] for n, _ in w.cases)
    assert set(per_edge) == {"tie", "root", "one", "flat", "sided", "absent", "all", "width", "limit", "wild", "quirk", "unpinned"} and min(per_edge.values()) >= 2
    print("tree edges: %d cases, per edge %s" % (len(w.cases), dict(per_edge)))
    empty = {n for n, t in w.cases if not w.want(n, t, 0, LAST)[0]}
    assert empty == EMPTY, (sorted(empty - EMPTY), sorted(EMPTY - empty))
    host.close()
