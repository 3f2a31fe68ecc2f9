"""Which of several documents of EQUAL weight an answer holds.  Every answer ends in a top-k under the reference's order — weight descending, docid
ascending on equal weights (msetcmp_by_relevance<true>) — and that order is written down separately in the bitonic sorts of the bodies, the disjunction's own
sort, the units' cut-offs, the query-wide histogram thresholds, the disjunction's second pass, the last-unit merge, the merge kernels, the shard merges and
the replay / count / frozen kernels.  On the synthetic corpus equal weights are accidents; here they are the rule: every document has the same length, so a
weight depends on the wdf vector alone, wdf is 1 or 2 (1 throughout for the two plateau terms), and the k-th rank of nearly every page lies inside a class of
bit-identical weights that spans stripes, units and shards.  A `<` written as `<=`, a unit dropped by weight alone or a shard merge that compares local docids
leave weights and ranks plausible and change only WHICH of the tied docids come back: every case is compared with the oracle at every rank (docid, weight bits,
subqs_matched), and tie_info() proves from the oracle alone that the case sits on a tie.  Also runs under the CPU emulation (tests/test_emu_ties.py)."""
import ctypes as C
import os
import random
import struct
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
from xapiand_amd import Database, Query, _lib, get_mset_sharded
from xapiand_amd.enquire import merged_stats, plan, search_batch, search_batch_replay, search_replay, search_sharded

pytestmark = [pytest.mark.gpu]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = bool(os.environ.get("XGM_EMU_QUICK"))
SB, W, N_STRIPES, N_SHARDS = 10, 1024, 8, 4
LAST = N_STRIPES * W - 1                   # docids 1 .. 8191: stripe = docid >> 10; containers from df >= 32 x 8 = 256
DOCLEN = 24                                # every document: its terms, then fillers up to this length
MAX_K = 1024                               # include/xgm.h: XGM_MAX_K
DENSE, PLATEAU, TAIL = ("d1", "d2", "d3"), ("p1", "p2"), ("l2", "lf", "l3")
RARE = ("r1", "r2", "r3", "r4", "r5", "r6")                     # one df: one term weight — documents that hold DIFFERENT rare terms tie as well
ORDER = PLATEAU + TAIL + DENSE + ("s67",) + RARE                # the order a document's terms stand in where they stand side by side (phrases match there)


def bits(w):
    return struct.unpack("<Q", struct.pack("<d", w))[0]


def make_postings():
    rng = random.Random(0x71ED)
    docs = range(1, LAST + 1)
    wdf = {t: {} for t in ORDER}
    for d in docs:
        for t, p in (("d1", 0.6), ("d2", 0.5), ("d3", 0.5)):
            if rng.random() < p: wdf[t][d] = 1 if rng.random() < 0.7 else 2
        for t in PLATEAU:
            if rng.random() < 0.5: wdf[t][d] = 1                   # the plateau: wdf 1 wherever they are, about 2000 documents hold both
        if d >> SB >= 6: wdf["s67"][d] = rng.randint(1, 2)         # every document of stripes 6 - 7 and no other
    # the long-tail terms mostly where the container terms are, so that conjunctions they lead still have classes of several members
    for t, n, among, m in (("l2", 150, DENSE, 50), ("l3", 100, DENSE[:2], 40)):
        for d in rng.sample([d for d in docs if all(d in wdf[x] for x in among)], n) + rng.sample(docs, m): wdf[t][d] = 1 if rng.random() < 0.6 else 2
    leads = sorted(set(wdf["l2"]) | set(wdf["l3"]))
    for d in rng.sample(leads, 225) + rng.sample([d for d in docs if d not in wdf["l2"] and d not in wdf["l3"]], 25):
        wdf["lf"][d] = 1 if rng.random() < 0.6 else 2              # a screen without containers: more postings than either lead, fewer than 256
    for t in RARE:
        for d in rng.sample(docs, 40): wdf[t][d] = 1
    post, doclen = {}, {}
    for d in docs:
        mine = [t for t in ORDER if d in wdf[t]]
        rest = [t for t in mine for _ in range(wdf[t][d] - 1)]
        assert len(mine) + len(rest) <= DOCLEN, d
        tail = rest + ["x%d" % rng.randrange(4) for _ in range(DOCLEN - len(mine) - len(rest))]
        if rng.random() < 0.5:                                     # half of the documents: their terms side by side in ORDER, the rest behind them
            rng.shuffle(tail)
            toks = mine + tail
        else:
            toks = mine + tail
            rng.shuffle(toks)
        doclen[d] = len(toks)
        where = {}
        for p, t in enumerate(toks, 1):
            where.setdefault(t, []).append(p)
        for t, pp in where.items():
            assert t[0] == "x" or len(pp) == wdf[t][d]
            post.setdefault(t, []).append((d, len(pp), pp))
    return post, doclen


def shard_postings(post, doclen, s):
    """Global docid g lives in shard (g - 1) % N_SHARDS under the local docid (g - 1) // N_SHARDS + 1 (multi.h's interleaving)."""
    loc = lambda g: (g - 1) // N_SHARDS + 1
    return ({t: [(loc(g), w, pp) for g, w, pp in pl if (g - 1) % N_SHARDS == s] for t, pl in post.items()},
            {loc(g): n for g, n in doclen.items() if (g - 1) % N_SHARDS == s})


class Ties:
    """The corpus on the device, the oracle beside it, and what the oracle says about a case's ties."""

    def __init__(self, c, db):
        self.c, self.db, self._full = c, db, {}

    def full(self, op, terms, nr=0, window=0):
        """The oracle's whole match in rank order (computed once per query)."""
        key = (op, tuple(terms), nr, window)
        if key not in self._full:
            self._full[key] = H.oracle_search(self.c, op, terms, 0, LAST, window, n_required=nr)[0]
        return self._full[key]

    def top_class(self, op, terms, nr=0, window=0):
        full = self.full(op, terms, nr, window)
        return sum(1 for _, w, _ in full if bits(w) == bits(full[0][1])) if full else 0

    def tie_info(self, op, terms, first, maxitems, nr=0, window=0):
        """(boundary, members, stripes): the oracle's first + maxitems + 1 hits — a BOUNDARY case where hits [k - 1] and [k], k = first + maxitems, carry
        the same weight bits —, and from its full match list how many documents share that weight and in how many stripes they live."""
        k = first + maxitems
        probe, _ = H.oracle_search(self.c, op, terms, first, maxitems + 1, window, n_required=nr)
        if not (len(probe) > k and bits(probe[k - 1][1]) == bits(probe[k][1])):
            return False, [], 0
        members = [d for d, w, _ in self.full(op, terms, nr, window) if bits(w) == bits(probe[k][1])]
        return True, members, len({d >> SB for d in members})


@pytest.fixture(scope="module")
def tied(built, tmp_path_factory):
    post, doclen = make_postings()
    c = H.ManualCorpus(post, doclen)
    df = {t: len(post[t]) for t in ORDER}
    assert all(df[t] >= 2 * 32 * N_STRIPES for t in DENSE + PLATEAU + ("s67",)) and all(df[t] < 32 * N_STRIPES for t in TAIL + RARE), df
    assert df["lf"] > df["l2"] > df["l3"] and len({df[t] for t in RARE}) == 1, df
    assert all(w in (1, 2) for t in DENSE + TAIL + ("s67",) for _, w, _ in post[t]) and all(w == 1 for t in PLATEAU + RARE for _, w, _ in post[t])
    assert set(doclen.values()) == {DOCLEN}
    both = {d for d, _, _ in post["p1"]} & {d for d, _, _ in post["p2"]}
    assert 1800 <= len(both) <= 2300 and {d >> SB for d in both} == set(range(N_STRIPES)), len(both)
    assert {d >> SB for d, _, _ in post["s67"]} == {6, 7} and df["s67"] == 2 * W
    db = Database(c.build_segment(str(tmp_path_factory.mktemp("ties") / "t.seg"), stripe_bits=SB))
    yield Ties(c, db)
    db.close()
    c.close()


@pytest.fixture(scope="module")
def tied_shards(built, tmp_path_factory):
    """The same documents in 4 docid-interleaved shards (built once per module)."""
    post, doclen = make_postings()
    d = tmp_path_factory.mktemp("tie_shards")
    shards = [H.ManualCorpus(*shard_postings(post, doclen, s)) for s in range(N_SHARDS)]
    dbs = [Database(c.build_segment(str(d / ("s%d.seg" % s)), stripe_bits=SB)) for s, c in enumerate(shards)]
    yield shards, dbs
    for x in dbs:
        x.close()
    for c in shards:
        c.close()


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------------
# (operator, terms, n_required, labels of the page shapes that are NOT boundary cases — every other shape of the query is listed as one)
CONJ = [("AND", ["d1", "d2"], 0, ""), ("AND", ["d1", "d2", "d3"], 0, ""), ("AND", ["d1", "d2", "d3", "p1"], 0, "k65 all"),      # the dense body
        ("AND", ["p1", "p2"], 0, ""),                                                                                           # (one weight class)
        ("AND", ["d1", "d2", "s67"], 0, "all"),                                                                                    # (every match in the last stripes)
        ("FILTER", ["d1", "d2", "d3"], 2, ""), ("FILTER", ["p1", "d3", "p2"], 1, "edge-1 edge all"),
        ("AND", ["l2", "d1"], 0, "all"), ("AND", ["l3", "d1", "d2"], 0, "all"), ("AND", ["l2", "d1", "d2", "d3"], 0, "edge all"),      # the flat body, a container screen
        ("AND", ["l2", "lf"], 0, "all"), ("AND", ["l3", "lf", "d1"], 0, "k10 k64 k100 p7 all"), ("AND", ["l2", "lf", "p1", "d1"], 0, "k64 k65 k100 edge all"),      # ... a flat screen
        ("FILTER", ["l2", "lf", "d1"], 1, "all"), ("FILTER", ["l3", "d1", "d2"], 2, "all"),
        ("AND", ["d1", "d2", "d3", "p1", "p2"], 0, "all")]                                                                         # 5 terms: the queue path
DISJ = [("OR", ["d1", "d2"], 0, ""), ("OR", ["p1", "p2"], 0, ""),                                                             # (the plateau pair: three weights in all)
        ("OR", ["s67", "r1"], 0, "k10"),                                                                                         # (a class of > 384 in one stripe; the best weights last)
        ("OR", ["d1", "d2", "d3"], 0, ""), ("OR", ["s67", "d1", "l2"], 0, "k1 k10"), ("OR", ["p1", "p2", "lf"], 0, ""),
        ("OR", ["d1", "d2", "d3", "l2", "lf"], 0, "k1 k10 p7"), ("OR", ["p1", "p2", "s67", "l3", "r1"], 0, "k1 k100"),
        ("OR", ["r1", "r2", "r3", "r4", "r5", "r6", "l2", "l3", "lf", "s67"], 0, "k1 k10"),                                           # > 8 terms: the other weighing path
        ("OR", ["r1", "r2", "r3", "r4", "r5", "r6", "p1", "p2", "d1", "l2"], 0, "k1 k10")]
POSITIONAL = [("PHRASE", ["p1", "p2"], 0, ""), ("PHRASE", ["p1", "p2", "d1"], 0, ""), ("PHRASE", ["d1", "d2"], 0, ""), ("PHRASE", ["d2", "d3", "s67"], 0, ""),
              ("PHRASE", ["l2", "lf"], 0, ""), ("PHRASE", ["lf", "d1"], 0, ""), ("NEAR", ["p2", "p1"], 3, "")]


def page_shapes(t, op, terms, nr=0):
    """(label, first, maxitems): pages of 1 / 10 / 64 / 65 / 100, one that straddles the edge of the top weight class (c members) and one that starts at it —
    where c + 10 fits the device path's k —, one inside the match, one larger than the match."""
    c, n = t.top_class(op, terms, nr), len(t.full(op, terms, nr))
    out = [("k1", 0, 1), ("k10", 0, 10), ("k64", 0, 64), ("k65", 0, 65), ("k100", 0, 100)]
    if 2 <= c and c + 10 <= MAX_K:
        out += [("edge-1", c - 1, 2), ("edge", c, 10)]
    out.append(("p7", 7, 10))
    if n + 5 <= MAX_K:
        out.append(("all", 0, n + 5))
    return out


def cases_of(t, table, quick_stride=3):
    out = []
    for i, (op, terms, nr, loose) in enumerate(table):
        shapes = page_shapes(t, op, terms, nr)
        if QUICK:
            shapes = shapes[i % quick_stride::quick_stride]
        out += [(op, terms, nr, label, first, maxitems, label not in loose.split()) for label, first, maxitems in shapes]
    return out


def check_ties(t, cases, operators, positional=False):
    """The conditions on the INPUTS: every case listed as a boundary case is one (and no other), at least three quarters of the cases are, and for every operator
    at least one boundary class has members in 6 of the 8 stripes.  Returns (boundary cases, widest class in members, widest in stripes)."""
    n_b, widest, stripes_of = 0, (0, 0), {}
    for op, terms, nr, label, first, maxitems, listed in cases:
        nr, window = (0, nr) if positional else (nr, 0)        # (the third field of a positional case is its window)
        b, members, ns = t.tie_info(op, terms, first, maxitems, nr, window)
        assert b == listed, ("boundary case" if listed else "not a boundary case", op, terms, label, first, maxitems)
        n_b += b
        widest = max(widest, (len(members), ns))
        stripes_of[op] = max(stripes_of.get(op, 0), ns)
    assert n_b * 4 >= len(cases) * 3, (n_b, len(cases))
    if not QUICK:
        assert all(stripes_of.get(op, 0) >= 6 for op in operators), stripes_of
    print("ties: %s: %d cases, %d boundary cases, widest boundary class %d members in %d stripes" % ("/".join(operators), len(cases), n_b, widest[0], widest[1]))
    return n_b, widest


def rows(hits):
    return [(h.docid, bits(h.weight), h.subqs_matched) for h in hits]


def orows(want):
    return [(d, bits(w), m) for d, w, m in want]


def check_batch_and_single(t, cases):
    """One launch over all the cases, then every case in a launch of its own (latency mode cuts a query into more units: other cuts, other merges)."""
    c, db = t.c, t.db
    plans = [plan(db, Query(op, terms, n_required=nr), first, maxitems) for op, terms, nr, _, first, maxitems, _ in cases]
    for (op, terms, nr, label, first, maxitems, _), p, (hits, hdr) in zip(cases, plans, search_batch(db, plans)):
        what = (op, terms, label, first, maxitems)
        want, oh = H.oracle_search(c, op, terms, first, maxitems, n_required=nr)
        (h1, hdr1), = search_batch(db, [p])
        for got, ghdr, how in ((hits, hdr, "batch"), (h1, hdr1, "single")):
            assert rows(got) == orows(want), (what, how, first_difference(rows(got), orows(want)))
            assert ghdr.matches_exact == oh.matches and ghdr.max_possible == oh.max_possible, (what, how, ghdr.matches_exact, oh.matches)
            if want:
                assert ghdr.max_attained == oh.max_attained, (what, how)


def first_difference(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return "rank %d: got %r, want %r" % (i, g, w)
    return "lengths %d / %d" % (len(got), len(want))


# ---- tests ------------------------------------------------------------------------------------------------------------------------------------------

def test_tied_conjunctions_vs_oracle(tied):
    """AND of 2 - 5 terms and FILTER through the dense body, the flat body (container screen, flat screen) and the queue path."""
    cases = cases_of(tied, CONJ)
    check_ties(tied, cases, ("AND", "FILTER"))
    check_batch_and_single(tied, cases)


def test_tied_disjunctions_vs_oracle(tied):
    """OR of 2, 3, 5 and 10 terms: the plateau pair; a boundary class with more than 384 members in ONE stripe, so that whatever range a unit has every
    document of it is a candidate and the candidate queue (XGM_ORW_CAND) goes through several scoring chunks; the term of stripes 6 - 7, whose documents
    raise the query-wide histogram threshold late; more than 8 terms (the other weighing path)."""
    cases = cases_of(tied, DISJ)
    check_ties(tied, cases, ("OR",))
    b, members, _ = tied.tie_info("OR", ["s67", "r1"], 0, 100)
    per_stripe = np.bincount([d >> SB for d in members], minlength=N_STRIPES)
    assert b and per_stripe.max() > 384, per_stripe
    assert len({bits(w) for _, w, _ in tied.full("OR", ["p1", "p2"])}) == 3
    check_batch_and_single(tied, cases)


def test_tied_mixed_launch(tied):
    """Dense-body, flat-body and queue-path conjunctions and disjunctions in one launch, every page on a tie."""
    mixed = [("AND", ["d1", "d2", "d3"], 0, "k10", 0, 10, True), ("AND", ["l2", "lf"], 0, "k10", 0, 10, True), ("AND", ["d1", "d2", "d3", "p1", "p2"], 0, "k64", 0, 64, True),
             ("OR", ["p1", "p2"], 0, "k100", 0, 100, True), ("AND", ["l3", "d1", "d2"], 0, "k1", 0, 1, True), ("AND", ["p1", "p2"], 0, "p7", 7, 10, True),
             ("OR", ["s67", "d1", "l2"], 0, "k65", 0, 65, True), ("FILTER", ["l2", "lf", "d1"], 1, "k10", 0, 10, True), ("AND", ["d1", "d2", "s67"], 0, "k100", 0, 100, True)]
    check_ties(tied, mixed, ())
    check_batch_and_single(tied, mixed)


def positional_cases(t):
    out = []
    for i, (op, terms, window, loose) in enumerate(POSITIONAL):
        shapes = [("k1", 0, 1), ("k10", 0, 10), ("k64", 0, 64), ("k65", 0, 65), ("p7", 7, 10)]
        if QUICK:
            shapes = shapes[i % 3::3]
        out += [(op, terms, window, label, first, maxitems, label not in loose.split()) for label, first, maxitems in shapes]
    return out


def test_tied_positional_vs_oracle(tied):
    """PHRASE of 2 - 3 terms on the plateau (one weight class) and on mixed terms, one NEAR: without replay bits (the histogram's query-wide threshold) against the
    oracle; with XGM_REPLAY_BATCH_FROZEN against the oracle in the reference's mode.  k = 65 is a page the listing and frozen kernels decline: that row comes
    back through the replay at collection time, and must be the same."""
    c, db = tied.c, tied.db
    cases = positional_cases(tied)
    check_ties(tied, cases, ("PHRASE", "NEAR"), positional=True)
    query = lambda op, terms, window: Query(op, terms, window=window)
    plans = [plan(db, query(op, terms, window), first, maxitems) for op, terms, window, _, first, maxitems, _ in cases]
    got = search_batch(db, plans)
    frozen = search_batch_replay(db, [plan(db, query(op, terms, window), first, maxitems, check_at_least=first + maxitems) for op, terms, window, _, first, maxitems, _ in cases])
    for (op, terms, window, label, first, maxitems, _), p, (hits, hdr), (page, fhdr, _) in zip(cases, plans, got, frozen):
        what = (op, terms, window, label)
        want, oh = H.oracle_search(c, op, terms, first, maxitems, window)
        assert rows(hits) == orows(want), (what, first_difference(rows(hits), orows(want)))
        H.check_matches(hdr.matches_exact, oh.matches, len(hits), what)
        assert hdr.max_possible == oh.max_possible, what
        (h1, hdr1), = search_batch(db, [p])
        assert rows(h1) == orows(want), (what, "single", first_difference(rows(h1), orows(want)))
        H.check_matches(hdr1.matches_exact, oh.matches, len(h1), what)
        ref, _ = H.oracle_search(c, op, terms, first, maxitems, window, reference_select_bug=True)
        assert orows(page) == orows(ref), (what, "frozen", first_difference(orows(page), orows(ref)))


def test_tied_conjunctions_counted_in_the_batch(tied):
    """The conjunctions' boundary cases with XGM_REPLAY_BATCH_COUNT (k = 65 is past what the counting kernels take: the fallback when the batch is collected):
    the oracle's page and exact match count; known_matching_docs equal to the one-query replay's and within the match.  oracle/xgm_oracle.cc keeps the
    reference's known_matching_docs inside its ProtoMSet but does not hand it out (its header has n_hits, max_subqs, matches and the two maxima), so the
    figure is not compared with the oracle directly."""
    c, db = tied.c, tied.db
    cases = [x for x in cases_of(tied, CONJ) if x[6]][::3 if QUICK else 1]
    assert any(first + maxitems == 65 for _, _, _, _, first, maxitems, _ in cases) or QUICK
    plans = [plan(db, Query(op, terms, n_required=nr), first, maxitems, check_at_least=first + maxitems) for op, terms, nr, _, first, maxitems, _ in cases]
    got = search_batch_replay(db, plans, replay=_lib.XGM_REPLAY_BATCH_COUNT)
    for (op, terms, nr, label, first, maxitems, _), p, (page, hdr, known) in zip(cases, plans, got):
        what = (op, terms, label, first, maxitems)
        want, oh = H.oracle_search(c, op, terms, first, maxitems, n_required=nr)
        assert orows(page) == orows(want), (what, first_difference(orows(page), orows(want)))
        assert hdr.matches_exact == oh.matches, (what, hdr.matches_exact, oh.matches)
        _, _, want_known = search_replay(db, p)
        assert known == want_known and known <= oh.matches, (what, known, want_known, oh.matches)


# (operator, terms, every shard sums the weights in one order: the answer over the shards is the unsharded one and the tied class has members in every shard)
SHARDED = [("AND", ["d1", "d2", "d3"], True), ("OR", ["d1", "d2", "p1", "p2"], True), ("AND", ["p1", "p2"], True), ("OR", ["p1", "p2"], True),
           # every shard plans with its own term frequencies, as the reference does: here one shard adds the four weights in another order and its
           # documents come out one ulp apart — the tied class is what the other three shards hold
           ("OR", ["d1", "d2", "d3", "p1"], False)]
SHARD_PAGES = [(0, 10), (7, 10)]


def sharded_cases(tied, shards):
    """(op, terms, first, maxitems, the oracle's page over the shards): every page ends inside a class of equal weights that has members in every shard, and
    the members the page holds do not all come from shard 0 — a merge that compared LOCAL docids, or preferred a shard, would hand out others."""
    out = []
    for op, terms, uniform in SHARDED:
        full = H.oracle_search_sharded(shards, op, terms, 0, LAST // N_SHARDS + 1)             # (every shard's whole match)
        for first, maxitems in SHARD_PAGES:
            k = first + maxitems
            probe = H.oracle_search_sharded(shards, op, terms, 0, k + 1)
            assert len(probe) > k and bits(probe[k - 1][1]) == bits(probe[k][1]), (op, terms, first, maxitems)
            members = sorted(d for d, w, _ in full if bits(w) == bits(probe[k][1]))
            want = probe[first:k]
            assert orows(want) == orows(H.oracle_search_sharded(shards, op, terms, first, maxitems))
            on_page = [d for d, _, _ in want if d in set(members)]
            assert on_page and {(g - 1) % N_SHARDS for g in on_page} != {0} and {(g - 1) % N_SHARDS for g in members[:N_SHARDS]} != {0}, (op, terms, on_page)
            if uniform:
                assert {(g - 1) % N_SHARDS for g in members} == set(range(N_SHARDS)), (op, terms, first, maxitems)
                assert orows(want) == orows(H.oracle_search(tied.c, op, terms, first, maxitems)[0][first:]), (op, terms)
            out.append((op, terms, first, maxitems, want))
    return out


def test_tied_shards_host_and_c_abi(tied, tied_shards):
    """get_mset_sharded (the host merge) and xgm_search_sharded (the C ABI: merge on the device) over 4 docid-interleaved shards."""
    shards, dbs = tied_shards
    cases = sharded_cases(tied, shards)
    for op, terms, first, maxitems, want in cases:
        mset = get_mset_sharded(dbs, Query(op, terms), first, maxitems)
        assert [(i.docid, bits(i.weight), i.subqs_matched) for i in mset] == orows(want), (op, terms, first, maxitems)
    for first, maxitems in SHARD_PAGES:
        sel = [x for x in cases if x[2:4] == (first, maxitems)]
        for (op, terms, _, _, want), mset in zip(sel, search_sharded(dbs, [Query(op, terms) for op, terms, _, _, _ in sel], first, maxitems)):
            assert [(i.docid, bits(i.weight), i.subqs_matched) for i in mset] == orows(want), (op, terms, first, maxitems)


def test_tied_shards_device_merge(tied, tied_shards):
    """xgm_search_batch_device + xgm_merge_shards_device (one array of hits and one of headers per shard) and the packed record (one per shard: [nq][k] hits,
    then [nq] headers) + xgm_merge_shards_packed_device."""
    import torch
    shards, dbs = tied_shards
    cases = sharded_cases(tied, shards)
    L = _lib.lib()
    for first, maxitems in SHARD_PAGES:
        sel = [x for x in cases if x[2:4] == (first, maxitems)]
        queries = [Query(op, terms) for op, terms, _, _, _ in sel]
        nq, k, n = len(sel), first + maxitems, len(dbs)
        all_hits = torch.zeros((n, nq, k, 2), dtype=torch.float64, device="cuda")
        all_hdrs = torch.zeros((n, nq, 4), dtype=torch.float64, device="cuda")
        rec_f64 = L.xgm_shard_record_bytes(nq, k) // 8
        assert rec_f64 == nq * (k * 2 + 4)
        all_rec = torch.zeros((n, rec_f64), dtype=torch.float64, device="cuda")
        for s, db in enumerate(dbs):
            arr = (_lib.Query * nq)(*[plan(db, qq, 0, k, global_stats=merged_stats(dbs, qq)) for qq in queries])
            _lib.check(L.xgm_search_batch_device(db._h, arr, nq, k, all_hits[s].data_ptr(), all_hdrs[s].data_ptr()))
            _lib.check(L.xgm_search_batch_device(db._h, arr, nq, k, all_rec[s].data_ptr(), all_rec[s].data_ptr() + nq * k * 16))
        torch.cuda.synchronize()
        ks = (C.c_uint32 * nq)(*([k] * nq))
        outs = []
        for packed in (False, True):
            out_hits = torch.zeros((nq, k, 2), dtype=torch.float64, device="cuda")
            out_hdrs = torch.zeros((nq, 4), dtype=torch.float64, device="cuda")
            if packed:
                _lib.check(L.xgm_merge_shards_packed_device(dbs[0]._h, all_rec.data_ptr(), n, nq, k, ks, out_hits.data_ptr(), out_hdrs.data_ptr()))
            else:
                _lib.check(L.xgm_merge_shards_device(dbs[0]._h, all_hits.data_ptr(), all_hdrs.data_ptr(), n, nq, k, ks, out_hits.data_ptr(), out_hdrs.data_ptr()))
            torch.cuda.synchronize()
            outs.append((packed, out_hits.cpu().numpy().view(np.uint8).reshape(nq, k, 16), out_hdrs.cpu().numpy().view(np.uint8).reshape(nq, 32)))
        for packed, raw, hdr in outs:
            for i, (op, terms, _, _, want) in enumerate(sel):
                nh = int(hdr[i, 0:4].view(np.uint32)[0])
                got = [(int(raw[i, j, 0:4].view(np.uint32)[0]), int(raw[i, j, 8:16].view(np.uint64)[0]), int(raw[i, j, 4:8].view(np.uint32)[0])) for j in range(nh)]
                assert got[first:] == orows(want), (op, terms, first, maxitems, "packed" if packed else "arrays")


# ---- the same conjunctions and disjunctions under the library's A/B switches (read once per process: a fresh child each) ----
SWITCHES = ["XGM_OR_SEED_SCALE=8", "XGM_OR_SEED_SCALE=1.3", "XGM_ORW_PLANES=4", "XGM_ORW_PLANES=6", "XGM_ORW_PLANES=4,XGM_OR_SEED_SCALE=8", "XGM_NO_OR_FLAT",
            "XGM_ORW2=1,XGM_OR_SEED_SCALE=8", "XGM_NO_PRUNE", "XGM_NO_FUSED_MERGE", "XGM_OR_FUSED_MERGE", "XGM_NO_FLAT", "XGM_NO_DENSE_BODY",
            "XGM_NO_ANDW,XGM_NO_ORW", "XGM_DENSE_KERNEL"]
_first_failure = []


@pytest.mark.parametrize("switch", SWITCHES)
def test_ties_under_kernel_variants(built, switch):
    """The second pass of the disjunction (a guess of the k-th weight far too high, a little too high), its plane counts, its terms through the block decode, the
    word-major kernel, no pruning; the merge launches instead of the last-unit merge, and the disjunction's opt-in last-unit merge; the queue path instead of the
    flat and the dense body; the workgroup kernels; the dense body as a kernel of its own.  One child after the other; after the first that fails none is started."""
    assert not _first_failure, "not run: %s" % _first_failure[0]
    env = dict(os.environ)
    for one in switch.split(","):
        name, _, val = one.partition("=")
        env[name] = val or "1"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_ties.py"), "-x", "-q", "-m", "gpu", "-k", "tied_conjunctions_vs or tied_disjunctions_vs",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        _first_failure.append("%s failed with %d:\n%s\n%s" % (switch, r.returncode, r.stdout[-3000:], r.stderr[-2000:]))
    assert r.returncode == 0 and "2 passed" in r.stdout, _first_failure[0] if _first_failure else r.stdout[-2000:]
