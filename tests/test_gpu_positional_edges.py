"""The positional filter (PHRASE, windowed PHRASE, NEAR) at the seams of its staging, on the crafted corpus of helpers.positional_edge_postings() and
the explicit table of helpers.positional_edge_cases(): the length of a term's list at every tier (at most 16 two-byte positions: staged 64 documents at
a time; 17 - 64: sixteen at a time, four lanes a list; more, or 4-byte lists: the serial predicates on the wave's copy), the deciding position at every
index a second load, a wide row or a copied chunk begins with, the long list under every plan term the kernels treat apart, rounds of 64 survivors made
of each kind and of all three, the 65 535 / 65 536 boundary with a 2-byte and a 4-byte term in one query, and the predicates' own edges (a word below
its phrase index, position 0, b - base == window, span == window - 1, a list that runs out).

A conjunction here is a GROUP of at most 64 consecutive docids (the `several` cases: two groups, 104 and 128 documents, asked at 192 only), so a page
of 64 (the bodies' largest) or of 192 (the wave kernel's queue path) is the whole match: no k-th weight forms and no candidate is dropped before its positions are tested — the tallying instantiation counts the positions of every
conjunction document.  Expectations: the CPU oracle, which tests/test_oracle_vs_reference.py and tests/golden/positional_edges.json pin to the compiled
reference on these very cases, and — for the verdict on every conjunction document — helpers.py_positional, a third statement of the three procedures.

The same file runs under the CPU emulation of the kernels with guard pages behind every device buffer (tests/test_emu_positional_edges.py)."""
import collections
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
from test_batch_plan import plan_dump
from xapiand_amd import Database, Query, _lib, plan, search_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = bool(os.environ.get("XGM_EMU_QUICK"))
SWITCHES = ("XGM_NO_DENSE_PHRASE_BODY", "XGM_NO_FLAT_PHRASE", "XGM_NO_PHRASEW", "XGM_NO_ANDW", "XGM_DENSE_KERNEL", "XGM_NO_FUSED_MERGE")
VARIANT = any(os.environ.get(s) for s in SWITCHES)
K_TABLE, K_BODY = 192, 64                          # the table's page (helpers.POS_EDGE_MAXITEMS: the wave kernel's queue path); the largest the bodies take
QF_DENSE, QF_FLAT = 64, 128                        # xgm_device.h
TF_POS_OK, TF_POS16, POS_PAD = 1, 2, 32            # xgm_segment.h
S_TERM_FLAGS, S_TERM_POS, S_POSITIONS, S_COUNT = 4, 7, 13, 16
EDGES = {"len", "len4", "idx", "round", "plan", "width", "exact", "window", "near", "several"}
WG_MAX_TERMS = 3                                   # XGM_PHRASE_MAX_TERMS_WG


class World:
    def __init__(self, d):
        self.post, self.doclen = H.positional_edge_postings()
        self.c = H.ManualCorpus(self.post, self.doclen)
        self.seg = self.c.build_segment(str(d / "pe.seg"), stripe_bits=8)
        self.db = Database(self.seg)
        self.cases = H.positional_edge_cases()
        self.info = H.positional_edge_term_info()
        self.lists = {c["name"]: H.positional_edge_lists(c) for c in self.cases}
        self.body_cases = [c for c in self.cases if len(self.lists[c["name"]][0]) <= K_BODY]          # all but `several`
        self._want = {}

    def want(self, case, maxitems):
        """The oracle's (rows, hdr): computed once per (case, page), shared by the tests, never changed."""
        key = (case["name"], maxitems)
        if key not in self._want:
            self._want[key] = H.oracle_search(self.c, case["op"], case["terms"], 0, maxitems, case["window"])
        return self._want[key]

    def plans(self, cases, maxitems, cal=0):
        return [plan(self.db, Query(c["op"], c["terms"], window=c["window"]), 0, maxitems, cal) for c in cases]

    def n_positions(self, cases):
        """Σ wdf of every query term over every conjunction document of every case."""
        return sum(len(pp) for c in cases for ls in self.lists[c["name"]][0].values() for pp in ls)

    def close(self):
        self.db.close()
        self.c.close()


@pytest.fixture(scope="module")
def world(built, tmp_path_factory):
    w = World(tmp_path_factory.mktemp("positional_edges"))
    yield w
    w.close()


def rows(hits):
    return [(h.docid, h.weight, h.subqs_matched) for h in hits]


def check_whole(w, case, hits, hdr, maxitems, what):
    want, oh = w.want(case, maxitems)
    assert rows(hits) == want, (case["name"], what, sorted(set(r[0] for r in rows(hits)) ^ set(r[0] for r in want))[:8])
    assert hdr.matches_exact == oh.matches == len(want), (case["name"], what, hdr.matches_exact, oh.matches)
    assert hdr.max_possible == oh.max_possible, (case["name"], what)
    if want:
        assert (hdr.max_attained, hdr.max_weight_subqs_matched) == (oh.max_attained, oh.max_subqs), (case["name"], what)
    return len(want)


def segment_sections(path):
    with open(path, "rb") as f:
        b = f.read()
    off = struct.unpack_from("<%dQ" % S_COUNT, b, 104)
    size = struct.unpack_from("<%dQ" % S_COUNT, b, 104 + 8 * S_COUNT)
    return b, off, size


def test_every_edge_has_cases(world):
    """The table is what it claims to be.  Every conjunction is its group (at most 64 documents, under the 150 a page of 192 must hold); on every
    conjunction document the Python restatement of the reference's procedures, the exhaustive search for what they look for (where it can be enumerated)
    and the oracle agree; every document crafted for a case has the verdict it was crafted for, and every cell has matches and near-misses.  The segment
    holds the positions as written (read back from the device), with 2-byte lists exactly where no position of the term reaches 65 536.

    Combinations that do not exist, and why:
      - a windowed phrase the greedy walk misses but a full search finds: there is none.  For a base the walk takes the smallest position of every later
        word in turn, so its chain is the pointwise smallest; a later base has a pointwise later chain, hence a `b` at least as large, hence it must be at
        least b - window: the restart skips nothing that could fit (asserted here by the exhaustive search on every document it can enumerate, among them
        the `skip` documents of the window groups, whose restart passes over a base).
      - NEAR with window 70 000 over 2-byte lists: a span of window - 1 needs a position past 65 535, so those terms have 4-byte lists (the serial path);
        the 2-byte tiers meet NEAR with windows n + 2 in the len, idx and plan cells.
      - the wide pass (17 - 64 positions, sixteen documents at a time) over 4-byte lists, and the bodies over 5 - 8 terms: the kernels have neither.
      - 4-byte lists of 8, 9, 32 ... positions: the serial copy has no tier below its 16-byte chunk; LEN32 holds the chunk's edges (4 | 5, 16 | 17, 64 | 65,
        252 | 253 | 254: the last full chunk, and the partial ones)."""
    w = world
    assert K_TABLE == H.POS_EDGE_MAXITEMS and all(c["maxitems"] == K_TABLE for c in w.cases)
    per_edge = collections.Counter(c["edge"] for c in w.cases)
    assert set(per_edge) == EDGES and min(per_edge.values()) >= 3, per_edge
    cells = collections.defaultdict(lambda: [0, 0])            # (edge, op tag, ...) -> [matching, near-miss] among the crafted documents
    seen_len, seen_idx = collections.defaultdict(set), collections.defaultdict(set)
    n_docs = n_enum = 0
    for c in w.cases:
        lists, intent = w.lists[c["name"]]
        conj, _ = H.oracle_search(w.c, "AND", c["terms"], 0, H.POS_EDGE_LASTDOCID)
        assert sorted(d for d, _, _ in conj) == sorted(lists) and len(lists) <= (H.POS_EDGE_MAX_CONJ if c["edge"] == "several" else K_BODY), c["name"]
        want, oh = w.want(c, K_TABLE)
        assert oh.matches == len(want), c["name"]
        matching = {d for d, _, _ in want}
        T = len(c["terms"])
        tag = "near" if c["op"] == "NEAR" else ("exact" if not c["window"] else "window")
        for d, ls in lists.items():
            assert len({p for pp in ls for p in pp}) == sum(len(pp) for pp in ls), (c["name"], d)       # distinct positions
            v = H.py_positional(c["op"], ls, c["window"])
            assert v == (d in matching), (c["name"], d, v)
            if T <= 3 or max(len(pp) for pp in ls) <= 70:
                assert H.full_search_positional(c["op"], ls, c["window"]) == v, (c["name"], d)
                n_enum += 1
            n_docs += 1
            if d in intent:
                assert intent[d] == v, (c["name"], d, intent[d])
                cells[(c["edge"], tag)][0 if v else 1] += 1
                wide4 = any(w.info[t]["wide"] for t in c["terms"])
                n = max(len(pp) for pp in ls)
                j = max(range(T), key=lambda i: len(ls[i]))
                seen_len[(c["edge"], tag, wide4, v)].add(n)
                if c["edge"] == "idx":                       # which entry of the long list stands next to the partner's single position
                    other = ls[1 - j][0]
                    seen_idx[(tag, n, v)].add(min(range(n), key=lambda i: abs(ls[j][i] - other)))
        assert not intent or ({True, False} <= set(intent.values())), c["name"]
    assert all(m > 0 and x > 0 for m, x in cells.values()), dict(cells)
    assert {(e, t) for e, t in cells} >= {(e, t) for e in ("len", "len4", "idx", "plan") for t in ("exact", "window", "near")}
    for tag in ("exact", "window", "near"):
        for v in (True, False):
            assert seen_len[("len", tag, False, v)] == set(H.LEN16), (tag, v)
            assert seen_len[("len4", tag, True, v)] == set(H.LEN32), (tag, v)
            assert seen_len[("plan", tag, False, v)] == {12, 20, 70}, (tag, v)
            for n in (16, 64, 254):
                assert seen_idx[(tag, n, v)] == {i for i in H.DECISIVE if i < n} | {n - 1}, (tag, n, v, sorted(seen_idx[(tag, n, v)]))
    assert {c["window"] - len(c["terms"]) for c in w.cases if c["edge"] == "window"} == {1, 3, 40}
    for T in (2, 3, 4, 6, 8):
        assert {c["window"] for c in w.cases if c["edge"] == "near" and len(c["terms"]) == T} == {T, T + 2, 40, 70000}
    assert sum(1 for c in w.cases if c["edge"] == "near" and len(c["terms"]) == 3 and c["window"] == 3) == 6          # every term order
    print("positional edges: %d cases %s; %d conjunction documents, %d of them also searched exhaustively" % (len(w.cases), dict(per_edge), n_docs, n_enum))
    # the segment: positions as written, the width of every term's lists, the 254-entry 4-byte list at the very end of the section
    L = _lib.lib()
    b, off, size = segment_sections(w.seg)
    names = w.c.terms()
    flags = struct.unpack_from("<%dI" % len(names), b, off[S_TERM_FLAGS])
    tpos = struct.unpack_from("<%dQ" % (len(names) + 1), b, off[S_TERM_POS])
    u32p = C.POINTER(C.c_uint32)
    for t, pl in w.post.items():
        tid, tf = C.c_uint32(), C.c_uint32()
        _lib.check(L.xgm_lookup_term(w.db._h, t.encode(), len(t), C.byref(tid), C.byref(tf), None, None))
        assert tf.value == len(pl) and names[tid.value] == t.encode()
        flat = [p for _, _, pp in sorted(pl) for p in pp]
        got = np.zeros(len(flat), dtype=np.uint32)
        assert L.xgm_debug_read_positions(w.db._h, tid.value, got.ctypes.data_as(u32p), got.size) == len(flat), (t, L.xgm_last_error())
        assert got.tolist() == flat, t
        assert flags[tid.value] & TF_POS_OK, t
        wide4 = max(flat) >= 65536
        assert bool(flags[tid.value] & TF_POS16) == (not wide4), t
        if t in w.info:
            assert w.info[t]["wide"] == wide4, t
            assert (len(pl) >= 480) == w.info[t]["dense"], (t, len(pl))
    last = names[-1].decode()
    assert last == "zz4rb" and w.info[last]["wide"] and len(sorted(w.post[last])[-1][2]) == 254
    assert tpos[-1] == tpos[-2] + 4 * sum(wdf for _, wdf, _ in w.post[last]) and size[S_POSITIONS] == tpos[-1] + POS_PAD
    want, _ = w.want(next(c for c in w.cases if c["name"] == "len4_zz4r_ex"), K_TABLE)
    assert sorted(w.post[last])[-1][0] in {d for d, _, _ in want}           # ... and its match, the list's last entry, is found


def test_whole_matches_vs_oracle(world):
    """The whole table in one batch — at the table's page of 192 (the wave kernel's own candidate queue) and at 64 (where the bodies take what they can),
    each with check_at_least = 0 (positions tested after the weight test) and with the exact count asked for — and every case alone: the oracle's rows,
    matches_exact equal to its count, unflagged: nothing was dropped untested."""
    w = world
    n = 0
    for k, cases in ((K_TABLE, w.cases), (K_BODY, w.body_cases)):
        for cal in (0, H.EXACT_COUNT):
            plans = w.plans(cases, k, cal)
            for c, (hits, hdr) in zip(cases, search_batch(w.db, plans)):
                n += check_whole(w, c, hits, hdr, k, ("batch", k, cal))
            if QUICK and (k, cal) != (K_BODY, 0):
                continue                                        # (emulated: every case alone once, where the bodies take it)
            for c, p in zip(cases, plans):
                (hits, hdr), = search_batch(w.db, [p])
                check_whole(w, c, hits, hdr, k, ("alone", k, cal))
    assert n > 4 * 2000


def test_bodies_took_the_queries(world):
    """Which code answered.  At a page of 64 with check_at_least = 0 a case of 2 - 4 terms that all have containers is the dense body's, one led by a
    rare term the flat body's, a case of 5 - 8 terms neither's; at 192 none is.  One launch of the positional instantiation either way.  The tallying
    instantiation counted the positions of every term in every conjunction document: all of them were tested."""
    if VARIANT:
        pytest.skip("the bodies of the default configuration")
    w = world
    qs = [Query(c["op"], c["terms"], window=c["window"]) for c in w.cases]
    _, flags, _ = plan_dump(w.db, qs, maxitems=K_BODY)
    n_by = collections.Counter()
    for c, f in zip(w.cases, flags):
        T = len(c["terms"])
        by_df = sorted(c["terms"], key=lambda t: len(w.post[t]))
        dense = T <= 4 and all(w.info[t]["dense"] for t in c["terms"])
        flat = T <= 4 and not w.info[by_df[0]]["dense"]
        assert bool(f & QF_DENSE) == dense and bool(f & QF_FLAT) == flat, (c["name"], f)
        n_by["dense" if dense else "flat" if flat else "queue"] += 1
    assert n_by["dense"] >= 40 and n_by["flat"] >= 40 and n_by["queue"] >= 15, n_by
    assert {len(c["terms"]) for c, f in zip(w.cases, flags) if not f & (QF_DENSE | QF_FLAT)} == {5, 6, 8}
    assert not any(f & (QF_DENSE | QF_FLAT) for f in plan_dump(w.db, qs, maxitems=K_TABLE)[1])
    for k, cases in ((K_BODY, w.body_cases), (K_TABLE, w.cases)):
        plans = w.plans(cases, k)
        arr = (_lib.Query * len(plans))(*plans)
        out = C.create_string_buffer(256)
        assert _lib.lib().xgm_debug_batch_launches(w.db._h, arr, len(plans), out, 256) == 1
        assert out.value.decode() == "xgm_andw_kernel:phrase*%d" % len(plans)
        w.db.set_profiling(2)
        got = search_batch(w.db, plans)
        tl = (C.c_uint64 * 10)()
        assert _lib.lib().xgm_last_batch_traffic(w.db._h, tl, 10) == 0
        w.db.set_profiling(0)
        for c, (hits, hdr) in zip(cases, got):
            check_whole(w, c, hits, hdr, k, ("tally", k))
        assert tl[7] == w.n_positions(cases), (k, tl[7], w.n_positions(cases))


def test_workgroup_kernel(world):
    """A page of 193 leaves the wave kernels for the workgroup kernel (xgm_match_kernel: a positional batch is never xgm_and_kernel's), which reads the
    positions straight from HBM: the cases of at most three terms, whose position-start tables fit a stripe whole, and a batch with a four- and an
    eight-term case, where the tables are sized for eight terms (at stripe_bits = 8 a stripe still fits: sub_bits stays 0, asserted)."""
    w = world
    small = [c for c in w.cases if len(c["terms"]) <= WG_MAX_TERMS]
    more = [c for c in w.cases if c["name"] in ("plan_p4d_win", "plan_p4f_near", "exact_ex8r", "near_n8r_w10_o1")]
    assert len(small) >= 80 and len(more) == 4
    for cases in (small, small[::7] + more):
        plans = w.plans(cases, 193)
        if not VARIANT:
            arr = (_lib.Query * len(plans))(*plans)
            out = C.create_string_buffer(256)
            assert _lib.lib().xgm_debug_batch_launches(w.db._h, arr, len(plans), out, 256) == 1
            assert out.value.decode() == "xgm_match_kernel*%d" % len(plans)
            sc, _, _ = plan_dump(w.db, [Query(c["op"], c["terms"], window=c["window"]) for c in cases], maxitems=193)
            assert sc["phrase"] == 1 and sc["sub_bits"] == 0 and sc["tab_terms"] == max(len(c["terms"]) for c in cases)
        for c, (hits, hdr) in zip(cases, search_batch(w.db, plans)):
            check_whole(w, c, hits, hdr, 193, "workgroup")


def test_top10_pages(world):
    """The same cases at a page of 10: the page is the oracle's, the count exact or a flagged lower bound that covers the page.  A group is one round of
    survivors, all weighed before any is held, so nothing of it is dropped; in the `several` cases a tenth-best weight stands when the second round
    arrives and candidates are dropped before their positions are tested — their counts are flagged (asserted: the pruning did run)."""
    w = world
    n_flagged = 0
    for cal in (0, H.EXACT_COUNT):
        for c, (hits, hdr) in zip(w.cases, search_batch(w.db, w.plans(w.cases, 10, cal))):
            want, oh = w.want(c, 10)
            assert rows(hits) == want, (c["name"], cal)
            if cal:
                assert hdr.matches_exact == oh.matches, (c["name"], hdr.matches_exact, oh.matches)
            else:
                H.check_matches(hdr.matches_exact, oh.matches, len(want), c["name"])
                n_flagged += bool(hdr.matches_exact & H.MATCHES_LOWER_BOUND)
    assert VARIANT or n_flagged >= 2, n_flagged


_first_failure = []


@pytest.mark.parametrize("switch", SWITCHES)
def test_edges_with_a_path_switched_off(built, switch):
    """The whole-match test once more per A/B switch (read once per process, hence the child): without the dense positional body, without the flat one,
    without the positional wave instantiation, without the conjunction wave kernel, on the stand-alone dense kernel, without the fused merge — whichever
    path takes a case over must give the same documents."""
    if QUICK:
        pytest.skip("one emulated process per switch is not a quick run")
    assert not _first_failure, "not run: %s" % _first_failure[0]          # one child after the other; after the first that fails none is started
    env = dict(os.environ, **{switch: "1"})
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                            "-k", "whole_matches_vs_oracle"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        _first_failure.append("%s: killed at its time limit:\n%s" % (switch, (e.stdout or b"")[-2000:]))
        raise AssertionError(_first_failure[0])
    if r.returncode != 0 or "1 passed" not in r.stdout:
        _first_failure.append("%s failed with %d:\n%s\n%s" % (switch, r.returncode, r.stdout[-3000:], r.stderr[-2000:]))
    assert not _first_failure, _first_failure[0]
