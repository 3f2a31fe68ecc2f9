"""Sorted and collapsed searches where their keys TIE and their buffers end.  Everything that is not plain relevance runs through one kernel,
xgm_match_sorted_kernel (xgm_match_body.inc compiled a second time; sorted_before, topk_sort_sorted, collapse_prune in xgm_kernels.hip), and one host merge
(sorted_batch_core in xgm_api.cc; the single entry points call it with nq = 1).  Its order — two 64-bit keys, then the docid ascending — is written down in
the kernel's sort, in its `take` test against the k-th entry and in the host's merge; its buffer has three sizes (512 / 1024 / 2048 entries for pages up to 256 / 768 / 1024); a collapse
key is collapsed in every unit and once more on the host.  On the synthetic corpus equal keys are accidents and no page is larger than about 300.

Here they are the rule: the documents of tests/test_gpu_ties.py (8 stripes x 1024 documents of one length, wdf 1 or 2: classes of bit-identical weights across
stripes, units and shards) with four value slots of this file's choosing (ManualCorpus.set_values):
    few   3 values, a quarter of the documents without one: classes of about 2000 documents in all 8 stripes
    uniq  every document its own value: the largest ordinal is the document count
    ckey  a collapse key: docid % 61 for three quarters of stripes 0 - 4 and 6 - 7, none for the rest, ONE key for all of stripe 5
    two   a collapse key of 2 values, no document without one: the collapsed match is at most 2 x collapse_max documents
Every case is compared with the oracle at every rank (docid, weight bits, subqs_matched, sort value, collapse key and count) and per search (match count,
best weight and its subqs_matched, collapsed lower bound), and the conditions on the INPUTS — that a case's page ends inside a class of equal keys, that a
collapse key's members lie in several stripes, ... — are proved from the oracle alone before anything is compared.  The oracle's sorted search is pinned to
the compiled reference (tests/test_oracle_vs_reference.py); its collapse is the intended semantics.
Also runs under the CPU emulation (tests/test_emu_sorted_ties.py)."""
import functools
import os
import subprocess
import sys

import pytest

import helpers as H
from test_gpu_ties import LAST, N_SHARDS, N_STRIPES, SB, W, bits, first_difference, make_postings, shard_postings
from xapiand_amd import Database, Query, _lib
from xapiand_amd.enquire import (merged_stats, plan, read_column_values, search_collapsed, search_collapsed_batch, search_filtered, search_sorted,
                                 search_sorted_batch, search_sorted_spy)

pytestmark = [pytest.mark.gpu]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = bool(os.environ.get("XGM_EMU_QUICK"))
UNITS_CAP = os.environ.get("XGM_MAX_UNITS_PER_QUERY")                # set in the child process of test_one_unit_per_query
DUMP = os.environ.get("XGM_SORTED_TIES_DUMP")                        # ... which leaves its answers here
MODES = {"V": _lib.XGM_SORT_VALUE, "VR": _lib.XGM_SORT_VALUE_RELEVANCE, "RV": _lib.XGM_SORT_RELEVANCE_VALUE, None: None}
FEW, UNIQ, CKEY, TWO = 0, 1, 2, 3
SLOT = {"few": FEW, "uniq": UNIQ, "ckey": CKEY, "two": TWO}


def make_values():
    """{slot: {docid: bytes}} from a fixed seed."""
    import random
    rng = random.Random(0x50D7)
    docs = list(range(1, LAST + 1))
    perm = docs[:]
    rng.shuffle(perm)
    few, uniq, ckey, two = {}, {}, {}, {}
    for d, r in zip(docs, perm):
        if rng.random() < 0.75: few[d] = rng.choice((b"a", b"b", b"c"))
        uniq[d] = b"%05d" % r                                      # (a permutation of 1 .. LAST: the ordinal of document d is int(uniq[d]))
        if d >> SB == 5: ckey[d] = b"S5"
        elif rng.random() < 0.75: ckey[d] = b"k%02d" % (d % 61)
        two[d] = b"x" if rng.random() < 0.5 else b"y"
    return {FEW: few, UNIQ: uniq, CKEY: ckey, TWO: two}


def shard_values(values, s):
    return {slot: {(g - 1) // N_SHARDS + 1: v for g, v in by.items() if (g - 1) % N_SHARDS == s} for slot, by in values.items()}


# ---- the tables -------------------------------------------------------------------------------------------------------------------------------------
# name: (operator, terms, n_required)
QUERIES = {"or2": ("OR", ["d1", "d2"], 0), "or3": ("OR", ["p1", "p2", "lf"], 0), "or5": ("OR", ["d1", "d2", "d3", "l2", "lf"], 0),
           "and2": ("AND", ["d1", "d2"], 0), "and5": ("AND", ["d1", "d2", "d3", "p1", "p2"], 0),
           "maybe": ("AND_MAYBE", ["p1", "d1", "d2"], 1), "not": ("AND_NOT", ["d1", "p2"], 1),
           "phrase": ("PHRASE", ["p1", "p2"], 0),                       # exact: the window is the number of terms
           "late": ("OR", ["s67", "r1"], 0),                            # the best weights come last in docid order
           "wide": ("OR", ["x0", "x1", "d1", "p1"], 0)}                 # (collapse cases only) the fillers: nearly every document matches
SORT_QUERIES = ["or2", "or3", "or5", "and2", "and5", "maybe", "not", "phrase", "late"]
# label: (first, maxitems).  The buffer: 512 entries up to k = 256, 1024 up to 768, 2048 up to 1024 (k = first + maxitems); p7 starts inside a tie class;
# "all" is larger than and5's match (asserted)
PAGES = {"k1": (0, 1), "k10": (0, 10), "k255": (0, 255), "k256": (0, 256), "k257": (0, 257), "k768": (0, 768), "k769": (0, 769), "k1024": (0, 1024),
         "p7": (7, 10), "p250": (250, 10), "all": (0, 400)}
PAGE_ORDER = ["k1", "k10", "k255", "k256", "k257", "k768", "k769", "k1024", "p7", "p250"]
# (mode, reverse, slot).  `uniq` never ties in its value: its cases are not boundary cases — what they add is the largest ordinal and, under RV, weights
# that tie in front of values that never do
SORTS = [("V", False, "few"), ("V", True, "few"), ("VR", False, "few"), ("VR", True, "few"), ("RV", False, "few"), ("RV", True, "few"),
         ("V", False, "two"), ("VR", True, "two"), ("RV", False, "two"), ("V", True, "ckey"), ("VR", False, "uniq"), ("RV", True, "uniq")]
# query: labels "page/mode+slot" (- = reverse) of the cases on slots few / two / ckey that are NOT boundary cases; every other case on these slots is listed
# as one, and no case on `uniq` is
LOOSE = {"or5": "k1/RV-few k1/RV+two k10/VR-few k256/RV+two k769/RV-few p7/RV+few p7/VR-two p250/RV-few p250/RV+two",      # (139 weights: small classes)
         "and5": "k256/RV+few k768/V+few k768/VR-few k768/V+two k768/V-ckey k769/V-few k769/RV+few k769/VR-two k1024/VR+few k1024/RV-few k1024/RV+two "
                 "p7/V-ckey all/VR+few all/RV-few all/RV+two",                                                                    # (282 matches: the pages beyond them)
         "not": "k256/V-ckey", "phrase": "k257/VR+few", "late": "k1/RV-few k257/V-ckey k1024/V+two"}
# (query, page) the library declines (XgmUnsupported): named here, never skipped silently — a case listed must be declined, every other answered.  None on
# this corpus: with stripes of 1024 documents even the phrase at k = 1024 keeps its tables and the 2048-entry buffer inside the 160 KiB of LDS
DECLINED = set()


def label_of(page, mode, rev, slot):
    return "%s/%s%s%s" % (page, mode, "-" if rev else "+", slot)


def sort_cases(quick=QUICK):
    """[(query, page, mode, reverse, slot name, listed as a boundary case)]: every query x page under 4 of the 12 sorts, rotated so that every (page, sort) pair
    comes up with three of the queries; and5 also with the page larger than its match."""
    out = []
    for qi, qn in enumerate(SORT_QUERIES):
        pages = PAGE_ORDER + (["all"] if qn == "and5" else [])
        for pi, pg in enumerate(pages):
            for si, (mode, rev, slot) in enumerate(SORTS):
                if si % 3 == (qi + pi) % 3:
                    out.append((qn, pg, mode, rev, slot, slot != "uniq" and label_of(pg, mode, rev, slot) not in LOOSE.get(qn, "").split()))
    return thin(out, 11, lambda c: (cap_of(*PAGES[c[1]]), c[2])) if quick else out


# (query, page, mode or None = by relevance, reverse, sort slot, collapse slot, collapse_max)
COLLAPSE = [("or2", "k10", None, False, "few", "ckey", 1), ("or2", "k256", None, False, "few", "ckey", 2), ("or3", "k257", "V", False, "few", "ckey", 1),
            ("wide", "k10", None, False, "few", "ckey", 1), ("wide", "k1024", None, False, "few", "ckey", 1), ("wide", "k769", "V", True, "few", "ckey", 3),
            ("and2", "p7", "RV", False, "few", "ckey", 2), ("or5", "k10", None, False, "few", "two", 1), ("or5", "k768", "VR", True, "few", "two", 3),
            ("phrase", "k10", None, False, "few", "ckey", 1), ("maybe", "k255", "V", False, "two", "ckey", 1), ("late", "k1024", None, False, "few", "ckey", 2),
            ("wide", "k257", "RV", True, "uniq", "ckey", 1), ("and5", "all", None, False, "few", "ckey", 1), ("or2", "k1024", "VR", False, "few", "ckey", 3),
            ("not", "k10", "V", True, "uniq", "ckey", 1), ("wide", "k1024", "V", False, "two", "ckey", 1), ("or3", "p250", None, False, "few", "ckey", 1)]


def collapse_cases(quick=QUICK):
    """Under emulation every third case — and always (wide, k1024, ckey): the only ones whose buffer of 2048 entries reaches collapse_prune's drop[4 .. 7]."""
    return thin(COLLAPSE, 3, lambda c: (cap_of(*PAGES[c[1]]), c[2] is None)) if quick else COLLAPSE


def cap_of(first, maxitems):
    k = first + maxitems
    return 512 if k <= 256 else 1024 if k <= 768 else 2048


def thin(cases, stride, cls):
    """Every stride-th case, and the first case of every class cls(case) that the stride left out."""
    keep = set(range(0, len(cases), stride))
    seen = {cls(cases[i]) for i in keep}
    for i, c in enumerate(cases):
        if cls(c) not in seen:
            keep.add(i); seen.add(cls(c))
    return [cases[i] for i in sorted(keep)]


def quick_searches():
    """How many searches the emulated run makes (tests/test_emu_sorted_ties.py takes its time limit from this)."""
    n_sort, n_col = len(sort_cases(True)), len(collapse_cases(True))
    return 2 * n_sort + 2 * n_col + 3 * len(SORT_QUERIES) + len(FILTERED[::3]) + 2 * len(TREE_CASES[::3]) + N_SHARDS * len(SHARDED[::2])


# ---- the corpus ------------------------------------------------------------------------------------------------------------------------------------

class World:
    """The corpus and its value slots in the oracle; on the device when `tmp` is given (column files of all four slots attached)."""

    def __init__(self, tmp=None):
        self.post, self.doclen = make_postings()
        self.values = make_values()
        self.c = H.ManualCorpus(self.post, self.doclen)
        for slot, by in self.values.items():
            self.c.set_values(slot, by)
        self.val = {slot: [by.get(d, b"") for d in range(LAST + 1)] for slot, by in self.values.items()}
        self._full, self._answers = {}, {}
        self.db, self.distinct = None, {}
        if tmp:
            self.db = Database(self.c.build_segment(os.path.join(tmp, "t.seg"), stripe_bits=SB))
            for slot in self.values:
                p = H.write_value_column(self.c, slot, os.path.join(tmp, "col%d" % slot))
                self.db.attach_column(p)
                self.distinct[slot] = read_column_values(p)
                assert self.distinct[slot] == sorted(set(self.values[slot].values()))

    def close(self):
        if self.db: self.db.close()
        self.c.close()

    def full(self, qn):
        """The oracle's whole match by relevance: [(docid, weight, subqs)]."""
        if qn not in self._full:
            op, terms, nr = QUERIES[qn]
            self._full[qn] = H.oracle_search(self.c, op, terms, 0, LAST, n_required=nr)[0]
        return self._full[qn]

    def oracle(self, qn, first, maxitems, mode, rev, slot, collapse=None):
        op, terms, nr = QUERIES[qn]
        return H.oracle_search_sorted(self.c, op, terms, first, maxitems, mode, SLOT[slot], rev, n_required=nr, collapse=collapse)

    def plan(self, qn, first, maxitems):
        op, terms, nr = QUERIES[qn]
        return plan(self.db, Query(op, terms, n_required=nr), first, maxitems)

    def key_of(self, slot, o):
        return self.distinct[SLOT[slot]][o - 1] if o else b""


@pytest.fixture(scope="module")
def world(built, tmp_path_factory):
    w = World(str(tmp_path_factory.mktemp("sorted_ties")))
    yield w
    w.close()


def tied(mode, a, b):
    """Two rows (docid, weight, subqs, sort key, ...) agree in every key compared before the docid."""
    return a[3] == b[3] and (mode == "V" or bits(a[1]) == bits(b[1]))


def boundary(w, qn, first, maxitems, mode, rev, slot):
    """(boundary case, stripes its class has members in, the oracle's page and header): the oracle's first + maxitems + 1 hits under the sort; a boundary case
    iff hits [k - 1] and [k], k = first + maxitems, agree in the value (V) / in value and weight bits (VR, RV).  The header does not depend on the page."""
    k = first + maxitems
    probe, hdr = w.oracle(qn, first, maxitems + 1, mode, rev, slot)
    if not (len(probe) > k and tied(mode, probe[k - 1], probe[k])):
        return False, 0, probe[:k], hdr
    val = w.val[SLOT[slot]]
    members = [d for d, x, _ in w.full(qn) if val[d] == probe[k][3] and (mode == "V" or bits(x) == bits(probe[k][1]))]
    assert probe[k - 1][0] in members and probe[k][0] in members
    return True, len({d >> SB for d in members}), probe[:k], hdr


def check_sort_inputs(w, cases, quick=QUICK):
    """The conditions on the inputs: listed equals computed for every case, at least three quarters are boundary cases, for every mode at least one boundary class
    has members in 6 of the 8 stripes, and5's match is smaller than its largest page.  Returns {case: (page, header)} of the oracle."""
    want, n_b, stripes_of = {}, 0, {}
    for case in cases:
        qn, pg, mode, rev, slot, listed = case
        b, ns, page, hdr = boundary(w, qn, *PAGES[pg], mode, rev, slot)
        assert b == listed, ("boundary case" if listed else "not a boundary case", qn, label_of(pg, mode, rev, slot))
        n_b += b
        stripes_of[mode] = max(stripes_of.get(mode, 0), ns)
        want[case[:5]] = (page, hdr)
    assert n_b * 4 >= len(cases) * 3, (n_b, len(cases))
    if not quick:
        assert all(stripes_of.get(m, 0) >= 6 for m in ("V", "VR", "RV")), stripes_of
        assert {cap_of(*PAGES[c[1]]) for c in cases} == {512, 1024, 2048}
    assert len(w.full("and5")) < sum(PAGES["all"])
    print("sorted ties: %d cases, %d boundary cases, widest class per mode in stripes %r" % (len(cases), n_b, stripes_of))
    return want


def hdr_row(hdr):
    return (hdr.n_hits, hdr.matches_exact, bits(hdr.max_attained), hdr.max_weight_subqs_matched)


def check_sorted_answer(w, what, slot, got, hdr, page, oh):
    """One device answer [(docid, weight, subqs, ordinal)] + header against the oracle's page [(docid, weight, subqs, key)] + header."""
    g, o = [(d, bits(x), m) for d, x, m, _ in got], [(d, bits(x), m) for d, x, m, _ in page]
    assert g == o, (what, first_difference(g, o))
    assert [w.key_of(slot, r[3]) for r in got] == [r[3] for r in page], what
    assert hdr.n_hits == len(page) and hdr.matches_exact == oh.matches, (what, hdr.n_hits, hdr.matches_exact, oh.matches)
    if page:
        assert (bits(hdr.max_attained), hdr.max_weight_subqs_matched) == (bits(oh.max_attained), oh.max_subqs), (what, hdr.max_attained, oh.max_attained)


def sorted_answers(w):
    """Every sort case through xgm_search_sorted, and through xgm_search_sorted_batch in one launch per (sort, buffer size) — a launch of more than 4 queries is
    planned with another merge budget than one query, so with other unit cuts: both against the oracle.  Returns the single searches' answers, serialised."""
    if "sorts" in w._answers:
        return w._answers["sorts"]
    cases = sort_cases()
    want = check_sort_inputs(w, cases)
    out, groups, declined = [], {}, set()
    for case in cases:
        qn, pg, mode, rev, slot, _ = case
        what = (qn, label_of(pg, mode, rev, slot))
        p = w.plan(qn, *PAGES[pg])
        if (qn, pg) in DECLINED:
            with pytest.raises(_lib.XgmUnsupported):
                search_sorted(w.db, p, MODES[mode], SLOT[slot], rev)
            declined.add((qn, pg))
            continue
        got, hdr = search_sorted(w.db, p, MODES[mode], SLOT[slot], rev)
        check_sorted_answer(w, what + ("single",), slot, got, hdr, *want[case[:5]])
        out.append((what, [(d, bits(x), m, o) for d, x, m, o in got], hdr_row(hdr)))
        groups.setdefault((mode, rev, slot, cap_of(*PAGES[pg])), []).append((case, p))
    assert declined == {x for x in DECLINED if any(c[:2] == x for c in cases)}
    assert QUICK or max(len(g) for g in groups.values()) > 4
    for (mode, rev, slot, _), members in groups.items():
        res = search_sorted_batch(w.db, [p for _, p in members], MODES[mode], SLOT[slot], rev)
        for (case, _), (got, hdr) in zip(members, res):
            check_sorted_answer(w, (case[0], label_of(*case[1:5]), "batch of %d" % len(members)), slot, got, hdr, *want[case[:5]])
    w._answers["sorts"] = repr(out).encode()
    return w._answers["sorts"]


def check_collapse_inputs(w, cases, quick=QUICK):
    """From the oracle alone: at least one page holds a key whose kept and dropped members lie in different stripes, one the stripe-5 key with a collapse count
    above 1000, one has fewer hits than its k while the match is larger, one mixes keyless and keyed documents at its last rank (the hit behind the page ties
    with the last one on it; one of the two has a key).  Returns {case: (page, header)}."""
    want, seen = {}, {"stripes": 0, "s5": 0, "short": 0, "mixed": 0}
    for case in cases:
        qn, pg, mode, rev, slot, cslot, cmax = case
        first, maxitems = PAGES[pg]
        k = first + maxitems
        probe, hdr = w.oracle(qn, first, maxitems + 1, mode, rev, slot, collapse=(SLOT[cslot], cmax))
        page = probe[:k]
        cval = w.val[SLOT[cslot]]
        on_page = {}
        for d, _, _, _, ck, cc in page:
            assert ck == cval[d]
            if ck: on_page.setdefault(ck, []).append(d)
        for ck, kept in on_page.items():
            cc = [r[5] for r in page if r[4] == ck][0]
            if cc and len(kept) == cmax:
                dropped = [d for d, _, _ in w.full(qn) if cval[d] == ck and d not in kept]
                assert len(dropped) == cc
                seen["stripes"] += bool({d >> SB for d in dropped} - {d >> SB for d in kept})
            seen["s5"] += ck == b"S5" and cc > 1000
        seen["short"] += len(probe) < k < hdr.matches
        if len(probe) > k:
            a, b = probe[k - 1], probe[k]
            seen["mixed"] += (bool(a[4]) != bool(b[4])) and (tied(mode, a, b) if mode else bits(a[1]) == bits(b[1]))
        want[case] = (page, hdr)
    if not quick:
        assert all(seen.values()), seen
        assert any(cap_of(*PAGES[c[1]]) == 2048 for c in cases)
    print("collapsed ties: %d cases, %r" % (len(cases), seen))
    return want


def check_collapsed_answer(w, what, slot, cslot, sorted_, got, hdr, clb, page, oh):
    g, o = [(d, bits(x), m) for d, x, m, _, _, _ in got], [(d, bits(x), m) for d, x, m, _, _, _ in page]
    assert g == o, (what, first_difference(g, o))
    assert [(w.key_of(cslot, co), cc) for _, _, _, _, co, cc in got] == [(ck, cc) for _, _, _, _, ck, cc in page], what
    if sorted_:
        assert [w.key_of(slot, r[3]) for r in got] == [r[3] for r in page], what
    assert hdr.n_hits == len(page) and hdr.matches_exact == oh.matches and clb == oh.collapsed_lower_bound, (what, hdr.n_hits, hdr.matches_exact, clb, oh.collapsed_lower_bound)
    if page:
        assert (bits(hdr.max_attained), hdr.max_weight_subqs_matched) == (bits(oh.max_attained), oh.max_subqs), what


def collapsed_answers(w):
    """Every collapse case through xgm_search_collapsed, and through xgm_search_collapsed_batch in a launch together with the same page and setting for five other
    queries (each of them against the oracle as well)."""
    if "collapse" in w._answers:
        return w._answers["collapse"]
    cases = collapse_cases()
    want = check_collapse_inputs(w, cases)
    out = []
    others = ["or2", "and2", "maybe", "not", "late"]
    for case in cases:
        qn, pg, mode, rev, slot, cslot, cmax = case
        what = (qn, pg, mode, rev, slot, cslot, cmax)
        p = w.plan(qn, *PAGES[pg])
        got, hdr, clb = search_collapsed(w.db, p, SLOT[cslot], cmax, MODES[mode], SLOT[slot], rev)
        check_collapsed_answer(w, what + ("single",), slot, cslot, mode, got, hdr, clb, *want[case])
        out.append((what, [(d, bits(x), m, o, co, cc) for d, x, m, o, co, cc in got], hdr_row(hdr), clb))
        names = [qn] + ([] if QUICK else [x for x in others if x != qn])
        res = search_collapsed_batch(w.db, [w.plan(x, *PAGES[pg]) for x in names], SLOT[cslot], cmax, MODES[mode], SLOT[slot], rev)
        for x, (got, hdr, clb) in zip(names, res):
            page, oh = want[case] if x == qn else w.oracle(x, *PAGES[pg], mode, rev, slot, collapse=(SLOT[cslot], cmax))
            check_collapsed_answer(w, (x,) + what[1:] + ("batch",), slot, cslot, mode, got, hdr, clb, page, oh)
    w._answers["collapse"] = repr(out).encode()
    return w._answers["collapse"]


# ---- tests ------------------------------------------------------------------------------------------------------------------------------------------

def test_value_slots_are_what_the_cases_need(world):
    w = world
    few, ckey = w.values[FEW], w.values[CKEY]
    for v in (b"a", b"b", b"c"):
        members = [d for d, x in few.items() if x == v]
        assert 1800 <= len(members) <= 2300 and {d >> SB for d in members} == set(range(N_STRIPES)), (v, len(members))
    assert 1800 <= LAST - len(few) <= 2300
    assert len(w.distinct[UNIQ]) == LAST == w.db.get_lastdocid()
    assert all(ckey[d] == b"S5" for d in range(5 << SB, 6 << SB)) and sum(1 for x in ckey.values() if x == b"S5") == W
    assert len(w.distinct[CKEY]) == 62 and 1500 <= LAST - len(ckey) <= 2100
    assert len(w.distinct[TWO]) == 2 and len(w.values[TWO]) == LAST


def test_sort_cases_vs_oracle(world):
    """Value sorts in three modes and both directions on four slots: OR of 2, 3 and 5 terms, AND of 2 and of 5, AND_MAYBE, AND_NOT, an exact PHRASE and the
    disjunction whose best weights come last; pages of 1, 10, around the three buffer sizes, inside a tie class and larger than the match."""
    a = sorted_answers(world)
    if DUMP:
        open(DUMP + ".sorts", "wb").write(a)


def test_collapse_cases_vs_oracle(world):
    """set_collapse_key by relevance and under the sorts: keys spread over every stripe, one key that owns a stripe (more members than the buffer holds: the
    fill shrinks to the survivors in the middle of the stripe), documents without a key, fewer collapsed hits than k."""
    a = collapsed_answers(world)
    if DUMP:
        open(DUMP + ".collapse", "wb").write(a)


def test_value_count_spy_on_tied_pages(world):
    """xgm_search_sorted_spy: the page of the plain sorted search; counts per value of three slots against the oracle's spy, their sum the match count."""
    w = world
    for qn in SORT_QUERIES:
        page, oh = w.oracle(qn, 0, 10, "V", False, "few")
        p = w.plan(qn, 0, 10)
        for spy in ("few", "ckey", "uniq"):
            total, want = H.oracle_spy(w.c, *QUERIES[qn][:2], SLOT[spy], n_required=QUERIES[qn][2])
            got, hdr, counts = search_sorted_spy(w.db, p, MODES["V"], FEW, False, SLOT[spy], len(w.distinct[SLOT[spy]]))
            check_sorted_answer(w, (qn, "spy", spy), "few", got, hdr, page, oh)
            assert hdr.matches_exact == total == sum(counts), (qn, spy)
            assert [(w.key_of(spy, o), n) for o, n in enumerate(counts) if o and n] == want, (qn, spy)
            assert counts[0] == total - sum(n for _, n in want), (qn, spy)


# (query, page, mode, reverse, slot): under a filter that lets through the documents whose `uniq` ordinal lies in [2048, 6144] — half of every tie class
FILTERED = [(qn, pg, mode, rev, slot) for qn in ("or2", "and2", "maybe", "late") for pg in ("k10", "k257", "k1024")
            for mode, rev, slot in (("V", False, "few"), ("VR", False, "two"), ("RV", False, "two"))]
F_LO, F_HI = 2048, 6144


def test_filtered_search_cuts_a_tie_class_in_two(world):
    """xgm_search_filtered under a sort: the oracle's full sorted list filtered on the host, cut to the page (dropping documents from a total order leaves the
    order of the rest).  Every page ends inside a class of equal keys of which the filter passes some members and drops others."""
    w = world
    ords = [0] + [int(w.values[UNIQ][d]) for d in range(1, LAST + 1)]
    ok = [F_LO <= o <= F_HI for o in ords]
    ok[0] = False
    flt = w.db.build_filter([(UNIQ, F_LO, F_HI)])
    assert flt.n_docs == sum(ok) == F_HI - F_LO + 1
    fulls = {}
    for qn, pg, mode, rev, slot in FILTERED[::3] if QUICK else FILTERED:
        what = (qn, label_of(pg, mode, rev, slot), "filtered")
        first, maxitems = PAGES[pg]
        k = first + maxitems
        if (qn, mode, rev, slot) not in fulls:
            fulls[(qn, mode, rev, slot)] = w.oracle(qn, 0, LAST, mode, rev, slot)[0]
        full = fulls[(qn, mode, rev, slot)]
        filtered = [r for r in full if ok[r[0]]]
        page = filtered[:k]
        assert len(filtered) > k and tied(mode, filtered[k - 1], filtered[k]), what
        members = [r[0] for r in full if tied(mode, r, filtered[k])]
        assert any(ok[d] for d in members) and not all(ok[d] for d in members), what
        got, hdr, _ = search_filtered(w.db, w.plan(qn, first, maxitems), flt, MODES[mode], SLOT[slot], rev)
        g, o = [(d, bits(x), m) for d, x, m, _ in got], [(d, bits(x), m) for d, x, m, _ in page]
        assert g == o, (what, first_difference(g, o))
        assert [w.key_of(slot, r[3]) for r in got] == [r[3] for r in page], what
        best = max(bits(r[1]) for r in filtered)
        msub = min((r[0], r[2]) for r in filtered if bits(r[1]) == best)[1]
        assert hdr_row(hdr) == (len(page), len(filtered), best, msub), (what, hdr_row(hdr), (len(page), len(filtered), best, msub))
    flt.close()


TREE = ("AND", ("OR", "d1", "p1"), ("OR", "d2", ("AND", "p2", "d3")))
TREE_CASES = [(pg, mode, rev, slot) for pg in ("k10", "k257", "k1024", "p7") for mode, rev, slot in (("V", False, "few"), ("VR", True, "few"), ("RV", True, "two"))]


def host_order(mode, rev):
    """The comparison of matcher/msetcmp.cc over rows (docid, weight, subqs, value bytes), as tests/helpers.py::oracle_search_sharded_sorted has it."""
    def cmp(a, b):
        if mode == "RV" and a[1] != b[1]:
            return -1 if a[1] > b[1] else 1
        if a[3] != b[3]:
            return (-1 if a[3] > b[3] else 1) if rev else (-1 if a[3] < b[3] else 1)
        if mode == "VR" and a[1] != b[1]:
            return -1 if a[1] > b[1] else 1
        return -1 if a[0] < b[0] else (1 if a[0] > b[0] else 0)
    return functools.cmp_to_key(cmp)


def test_nested_tree_under_a_sort(world):
    """A nested query: the oracle's tree evaluator has no sorted form, so its full relevance ranking is re-ranked under the comparison on the host."""
    w = world
    full, _, _ = H.oracle_search_tree(w.c, TREE, 0, LAST)
    assert len(full) > 1024 + 1
    for pg, mode, rev, slot in TREE_CASES[::3] if QUICK else TREE_CASES:
        what = ("tree", label_of(pg, mode, rev, slot))
        first, maxitems = PAGES[pg]
        k = first + maxitems
        val = w.val[SLOT[slot]]
        ranked = sorted([(d, x, m, val[d]) for d, x, m in full], key=host_order(mode, rev))
        assert tied(mode, ranked[k - 1], ranked[k]), what
        p = plan(w.db, Query.tree(TREE), first, maxitems)
        for how in ("single", "batch"):
            if how == "single":
                got, hdr = search_sorted(w.db, p, MODES[mode], SLOT[slot], rev)
            else:
                (got, hdr), _ = search_sorted_batch(w.db, [p, w.plan("or2", first, maxitems)], MODES[mode], SLOT[slot], rev)
            g, o = [(d, bits(x), m) for d, x, m, _ in got], [(d, bits(x), m) for d, x, m, _ in ranked[:k]]
            assert g == o, (what, how, first_difference(g, o))
            assert [w.key_of(slot, r[3]) for r in got] == [r[3] for r in ranked[:k]], (what, how)
            assert hdr.matches_exact == len(full) and bits(hdr.max_attained) == max(bits(x) for _, x, _ in full), (what, how)


# (query, page, mode, reverse, slot) over the 4 shards; OR and AND only (the sharded oracle takes no n_required)
SHARDED = [("or2", "k10", "V", False, "few"), ("and2", "p7", "VR", True, "few"), ("or3", "k10", "RV", False, "two"), ("or2", "k257", "V", True, "ckey"),
           ("or3", "k10", "VR", False, "two"), ("and2", "k10", "RV", True, "few")]


@pytest.fixture(scope="module")
def shard_worlds(built, tmp_path_factory):
    """The same documents in 4 docid-interleaved shards, each with its own column files (ordinals are per shard)."""
    post, doclen = make_postings()
    values = make_values()
    d = tmp_path_factory.mktemp("sorted_tie_shards")
    shards, dbs, distinct = [], [], []
    for s in range(N_SHARDS):
        c = H.ManualCorpus(*shard_postings(post, doclen, s))
        db = Database(c.build_segment(str(d / ("s%d.seg" % s)), stripe_bits=SB))
        mine = {}
        for slot, by in shard_values(values, s).items():
            c.set_values(slot, by)
            p = H.write_value_column(c, slot, str(d / ("s%d_col%d" % (s, slot))))
            db.attach_column(p)
            mine[slot] = read_column_values(p)
        shards.append(c); dbs.append(db); distinct.append(mine)
    yield shards, dbs, distinct
    for x in dbs:
        x.close()
    for c in shards:
        c.close()


def test_sorted_pages_of_four_shards_merged_by_value_strings(shard_worlds):
    """Xapiand's per-shard protocol under a value sort: every shard searched with the merged statistics and its own columns, the pages merged on the host by the
    value STRINGS under the same comparison, against the oracle's sharded sorted search.  Every page ends inside a class of equal keys with members in
    several shards."""
    shards, dbs, distinct = shard_worlds
    for qn, pg, mode, rev, slot in SHARDED[::2] if QUICK else SHARDED:
        what = (qn, label_of(pg, mode, rev, slot), "shards")
        op, terms, _ = QUERIES[qn]
        first, maxitems = PAGES[pg]
        k = first + maxitems
        probe = H.oracle_search_sharded_sorted(shards, op, terms, 0, k + 1, mode, SLOT[slot], rev)
        assert len(probe) > k and tied(mode, probe[k - 1], probe[k]), what
        assert len({(r[0] - 1) % N_SHARDS for r in probe if tied(mode, r, probe[k])}) > 1, what
        want = H.oracle_search_sharded_sorted(shards, op, terms, first, maxitems, mode, SLOT[slot], rev)
        assert want == probe[first:k]
        query = Query(op, terms)
        gs = merged_stats(dbs, query)
        rows = []
        for s, db in enumerate(dbs):
            got, _ = search_sorted(db, plan(db, query, 0, k, global_stats=gs), MODES[mode], SLOT[slot], rev)
            rows += [((d - 1) * N_SHARDS + s + 1, x, m, distinct[s][SLOT[slot]][o - 1] if o else b"") for d, x, m, o in got]
        rows.sort(key=host_order(mode, rev))
        g, o = [(d, bits(x), m, v) for d, x, m, v in rows[first:k]], [(d, bits(x), m, v) for d, x, m, v in want]
        assert g == o, (what, first_difference(g, o))


def test_one_unit_per_query(world):
    """The same sort and collapse cases in a child process with XGM_MAX_UNITS_PER_QUERY=1 (read once per process): one unit per query, so the host's merge has one
    list and its second collapse nothing to do — the kernel's buffer, thresholds and collapse do everything.  The child checks every case against the oracle;
    its answers must be byte-identical to those of the default cut."""
    if UNITS_CAP:
        return                                                      # (a child does not start children)
    import tempfile
    ours = {"sorts": sorted_answers(world), "collapse": collapsed_answers(world)}
    with tempfile.TemporaryDirectory() as tmp:
        dump = os.path.join(tmp, "answers")
        env = dict(os.environ, XGM_MAX_UNITS_PER_QUERY="1", XGM_SORTED_TIES_DUMP=dump)
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", "sort_cases_vs or collapse_cases_vs",
                            "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "2 passed" in r.stdout, "XGM_MAX_UNITS_PER_QUERY=1 failed with %d:\n%s\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-2000:])
        for name, mine in ours.items():
            theirs = open(dump + "." + name, "rb").read()
            assert len(mine) > 1000 and theirs == mine, (name, len(theirs), len(mine))
