"""xgm_dense_unit on stripes crowded with matches (>= 48 documents of the AND): wdf = 1 is read per document off the containers' wdf >= 2 planes instead of
the 128-slot summary — for the terms that hold no posting of wdf 0 (xgm_seg_dev::dense_wdf0; a clear plane bit says wdf 0 OR 1).  Hand-made documents on 8
stripes of 1024.  The planner cuts so small a shard into units of ONE stripe, so everything also runs in child processes with XGM_MAX_UNITS_PER_QUERY=1
(one unit of all 8 stripes) and =2 (two of 4), the spans asserted through xgm_debug_plan_batch: crowded and sparse stripes inside one unit, a threshold
formed in stripe 0 before the crowded stripes 2, 4, 6 (the class prefilter's planes), the stripe without a container between two crowded ones:

  stripe 0   crowded, the unit's first: no threshold yet, the new code loads the planes     stripe 4   crowded; the seam slots 0, 31 / 32, 127 / 128, W - 1
  stripe 1   30 documents of any AND with `a`: the summary rule, inside the same unit       stripe 5   sparse
  stripe 2   crowded; slots 256 .. 383 all match: one lane's 128 documents (the packed      stripe 6   `s` meets a, b and zm in 54 documents (<= 8 per aligned 128):
             code holds 16 of them, the rest consult the summary)                                      the tallies' one crowded stripe
  stripe 3   `a` has no posting: no container, next to two crowded stripes                  stripe 7   sparse

a b c d: frequent, wdf from {1, 2..4, 254}.  z0: every posting boolean (wdf 0).  zm: a few wdf 0 among wdf 1 and >= 2.  s: ~40 postings a stripe.
e1 e2: the run, the seam slots and docid 1 in short documents, wdf 1..3, among long documents of wdf 1 — the short ones ARE the first page of `e1 e2`.
Against the oracle at every rank: docid, weight bit pattern, subqs_matched, match count, maxima; the flags against the postings; the tallies against counts
derived from the postings; the switches in child processes.  Also runs under the CPU emulation (tests/test_emu_exact_wdf.py)."""
import ctypes as C
import os
import random
import subprocess
import sys

import pytest

import helpers as H
from xapiand_amd import Database, Query, _lib
from xapiand_amd.enquire import plan, search_batch

pytestmark = [pytest.mark.gpu]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = bool(os.environ.get("XGM_EMU_QUICK"))
SB, W, N_STRIPES = 10, 1024, 8
LAST = N_STRIPES * W - 1
FREQ, ORDER = ("a", "b", "c", "d"), ("s", "e1", "e2", "zm", "z0", "a", "b", "c", "d")
CROWDED, SPARSE, NO_A, TALLY_S = (0, 2, 4, 6), (1, 5, 7), 3, 6
EXACT_MIN = 48                             # XGM_DENSE_EXACT_MIN's default: matches of the AND in a stripe, before the prefilter
NO_EXACT, NO_SUM = bool(os.environ.get("XGM_NO_EXACT_WDF")), bool(os.environ.get("XGM_NO_WDF_SUMMARY"))
UNITS_CAP = os.environ.get("XGM_MAX_UNITS_PER_QUERY")                # set in the child processes of test_units_spanning_stripes
SPANS = {"1": [(0, 8)], "2": [(0, 4), (4, 8)]}
SEAMS = (0, 31, 32, 127, 128, W - 1)
RUN = range(2 * W + 256, 2 * W + 384)      # 128 consecutive docids, one lane's documents of stripe 2
D254 = 4 * W + 127


def draw_wdf(rng):
    x = rng.random()
    return 1 if x < 0.6 else (254 if x > 0.995 else rng.randint(2, 4))


def make_postings():
    """{term: {docid: wdf}}.  Nothing here depends on the code under test."""
    rng = random.Random(0xE8AC7)
    wdf = {t: {} for t in ORDER}
    for d in range(1, LAST + 1):
        s = d >> SB
        for t in FREQ:
            if t == "a" and s in SPARSE + (NO_A,):
                continue
            if rng.random() < 0.75: wdf[t][d] = draw_wdf(rng)
        if rng.random() < 0.8: wdf["z0"][d] = 0
        if rng.random() < 0.7: wdf["zm"][d] = 0 if rng.random() < 0.02 else draw_wdf(rng)
    for s in SPARSE:                                               # 30 documents a sparse stripe that hold every frequent term
        for d in rng.sample(range(s * W, (s + 1) * W), 30):
            for t in FREQ + ("z0", "zm"): wdf[t][d] = 0 if t == "z0" else draw_wdf(rng)
    for d in list(RUN) + [4 * W + x for x in SEAMS] + [1]:         # the run, the seams, docid 1: members of everything
        for t in FREQ + ("zm",): wdf[t][d] = draw_wdf(rng)
        wdf["z0"][d] = 0
    wdf["a"][4 * W] = 2; wdf["a"][4 * W + 31] = 1; wdf["a"][4 * W + 32] = 3; wdf["b"][4 * W + 128] = 2; wdf["c"][4 * W + W - 1] = 4; wdf["b"][1] = 2
    wdf["d"][D254] = 254
    wdf["zm"][2 * W + 300] = 0; wdf["zm"][2 * W + 260] = 0; wdf["zm"][4 * W + 128] = 0      # boolean postings inside the run (one past the packed code's 16) and at a seam
    # s: 54 documents of stripe 6 with a, b and zm, at most 7 in any aligned run of 128; elsewhere where `a` is absent, but for one document a stripe
    for blk in range(8):
        for d in rng.sample(range(TALLY_S * W + 128 * blk, TALLY_S * W + 128 * blk + 128), 7 if blk < 6 else 6):
            wdf["s"][d] = 1 + (d % 3 == 0)
            for t in ("a", "b", "zm"): wdf[t][d] = draw_wdf(rng)
    wdf["zm"][min(d for d in wdf["s"] if d >> SB == TALLY_S)] = 0   # ... one of them a boolean posting of zm
    for s in range(N_STRIPES):
        if s == TALLY_S:
            continue
        lo = max(1, s * W)
        free = [d for d in range(lo, (s + 1) * W) if d not in wdf["a"] and d not in RUN]
        for d in rng.sample(free, 38): wdf["s"][d] = 1
        if s != NO_A and s not in SPARSE:
            d = rng.choice([x for x in range(lo, (s + 1) * W) if x in wdf["a"] and x not in RUN and (x & (W - 1)) not in SEAMS and x != 1])
            wdf["s"][d] = 2
            for t in ("b", "zm"): wdf[t].setdefault(d, 1)
    # e1, e2: the same documents.  SPECIAL ones (short, wdf 1..3): the seams, docid 1, the run's slots 0..7 and 16..40; the others long with wdf 1 — a
    # weight grows with the wdf and falls with the length, so every special document outranks every other one
    special = [4 * W + x for x in SEAMS] + [1] + [RUN[i] for i in list(range(8)) + list(range(16, 41))]
    others = [d for d in RUN if d not in special] + rng.sample(range(2, W), 60) + rng.sample([4 * W + x for x in range(W) if x not in SEAMS], 60)
    for s_ in (1, 3, 5, 6, 7): others += rng.sample(range(s_ * W, (s_ + 1) * W), 10)
    for d in others:
        wdf["e1"][d] = wdf["e2"][d] = 1; wdf["z0"][d] = 0
    for d in special:
        wdf["e1"][d] = rng.choice((1, 1, 2, 3)); wdf["e2"][d] = rng.choice((1, 1, 2, 3)); wdf["z0"][d] = 0
    for d, w1, w2 in ((4 * W, 2, 1), (4 * W + 31, 1, 1), (4 * W + 32, 3, 1), (4 * W + 127, 1, 2), (4 * W + 128, 1, 1), (4 * W + W - 1, 1, 3), (1, 2, 1), (RUN[16], 1, 1), (RUN[17], 2, 1)):
        wdf["e1"][d], wdf["e2"][d] = w1, w2
    post, doclen = {t: sorted(wdf[t].items()) for t in ORDER}, {}
    for d in range(1, LAST + 1):
        doclen[d] = sum(wdf[t].get(d, 0) for t in ORDER) + rng.randint(3, 40) + (150 if d in wdf["e1"] else 0)
    for d in special: doclen[d] = 5 + rng.randint(0, 2)
    return wdf, post, doclen, special


class Shard:
    pass


@pytest.fixture(scope="module")
def shard(built, tmp_path_factory):
    wdf, post, doclen, special = make_postings()
    c = H.ManualCorpus(post, doclen, positions=False)
    sh = Shard()
    sh.c, sh.wdf, sh.special = c, wdf, special
    df = {t: len(post[t]) for t in ORDER}
    assert all(df[t] >= 32 * N_STRIPES for t in ORDER) and df["e1"] == df["e2"] < df["s"] < df["zm"] < df["z0"], df
    assert not any(d >> SB == NO_A for d in wdf["a"]) and set(wdf["z0"].values()) == {0} and {0, 1, 2} <= set(wdf["zm"].values())
    assert max(max(v.values()) for v in wdf.values()) == 254
    sh.db = Database(c.build_segment(str(tmp_path_factory.mktemp("exactwdf") / "s.seg"), stripe_bits=SB))
    sh.tid = {}
    for t in ORDER:
        tid, tf = C.c_uint32(), C.c_uint32()
        _lib.check(_lib.lib().xgm_lookup_term(sh.db._h, t.encode(), len(t), C.byref(tid), C.byref(tf), None, None))
        sh.tid[t] = tid.value
    yield sh
    sh.db.close()
    c.close()


def matches_per_stripe(sh, terms):
    docs = set.intersection(*(set(sh.wdf[t]) for t in terms))
    return [sum(1 for d in docs if d >> SB == s) for s in range(N_STRIPES)]


def test_the_corpus_holds_what_the_cases_need(shard):
    sh = shard
    for terms in (["a", "b"], ["a", "b", "c"], ["a", "b", "c", "d"], ["z0", "a", "b"], ["zm", "a", "b"]):
        n = matches_per_stripe(sh, terms)
        assert all(n[s] >= EXACT_MIN for s in (0, 2, 4)) and all(1 <= n[s] < EXACT_MIN for s in SPARSE) and n[NO_A] == 0, (terms, n)
    assert all(all(d in sh.wdf[t] for d in RUN) for t in FREQ + ("z0", "zm"))
    assert any(sh.wdf["a"][d] >= 2 for d in list(RUN)[16:]) and any(sh.wdf["a"][d] == 1 for d in list(RUN)[16:])
    for terms in TALLY_Q:
        n = matches_per_stripe(sh, terms)
        assert EXACT_MIN <= n[TALLY_S] <= 60 and sum(n) <= 64 and all(x < EXACT_MIN for s, x in enumerate(n) if s != TALLY_S), (terms, n)
        docs = set.intersection(*(set(sh.wdf[t]) for t in terms))
        assert max(sum(1 for d in docs if d >> 7 == blk) for blk in range((LAST >> 7) + 1)) <= 8


def test_wdf0_flags_against_the_postings(shard):
    sh = shard
    for t in ORDER:
        out = C.c_uint32(0xDEADBEEF)
        rc = _lib.lib().xgm_debug_read_term_wdf0(sh.db._h, sh.tid[t], C.byref(out))
        assert rc == 1 and out.value == (1 if 0 in sh.wdf[t].values() else 0), (t, rc, out.value)
    assert 0 in sh.wdf["z0"].values() and 0 in sh.wdf["zm"].values() and not any(0 in sh.wdf[t].values() for t in FREQ + ("s",))
    out = C.c_uint32(0)
    assert _lib.lib().xgm_debug_read_term_wdf0(sh.db._h, 1 << 30, C.byref(out)) < 0                  # term id out of range


PAGES = (1, 10, 64)
MIXED_Q = [["a", "b"], ["a", "c"], ["a", "b", "c"], ["b", "c", "d"], ["a", "b", "c", "d"]]
TRAP_Q = [["z0", "a", "b"], ["zm", "a", "b"], ["z0", "zm", "a"], ["z0", "zm", "a", "b"], ["z0", "a"]]
TALLY_Q = [["s", "a", "b"], ["s", "a", "zm"]]


def cases():
    qs = MIXED_Q + TRAP_Q + TALLY_Q
    return [(terms, k) for i, terms in enumerate(qs) for k in (PAGES if not QUICK else PAGES[i % 3:][:1])]


def test_conjunctions_vs_oracle(shard):
    """Mixed wdf, the wdf-0 trap, the seams and the run of 128: the batch call — tallying and plain instantiations — and each query alone.  In the children of
    test_units_spanning_stripes a unit holds crowded and sparse stripes, and stripe 0 is crowded before a threshold exists, stripes 2, 4, 6 after."""
    sh = shard
    cs = cases()
    plans = [plan(sh.db, Query("AND", terms), 0, k) for terms, k in cs]
    sh.db.set_profiling(2)
    tallied = search_batch(sh.db, plans)
    sh.db.set_profiling(0)
    plain = search_batch(sh.db, plans)
    for (terms, k), p, (hits, hdr), (hits0, hdr0) in zip(cs, plans, tallied, plain):
        what = (terms, k)
        want, oh = H.oracle_search(sh.c, "AND", terms, 0, k)
        assert [(h.docid, h.weight, h.subqs_matched) for h in hits0] == want, what
        assert [(h.docid, h.weight, h.subqs_matched) for h in hits] == want, what
        assert hdr.matches_exact == oh.matches and hdr0.matches_exact == oh.matches and hdr0.max_possible == oh.max_possible, what
        assert want and hdr0.max_attained == oh.max_attained, what
        (h1, hdr1), = search_batch(sh.db, [p])
        assert [(h.docid, h.weight, h.subqs_matched) for h in h1] == want and hdr1.matches_exact == oh.matches and hdr1.max_attained == oh.max_attained, what


def test_seams_and_the_run(shard):
    """Candidates at docid 1, slots 0, 31 / 32, 127 / 128, W - 1 of a crowded stripe and the run of 128 matches in one lane's documents (slots 16..40 of it lie
    past the 16 candidates the lane's packed code holds): they are the first page, so every one of them is compared."""
    sh = shard
    for terms in (["e1", "e2"], ["e1", "e2", "z0"]):
        n = matches_per_stripe(sh, terms)
        assert n[2] >= 128 and n[4] >= EXACT_MIN and n[0] >= EXACT_MIN and all(1 <= n[s] < EXACT_MIN for s in (1, 3, 5, 6, 7)), n
        want, oh = H.oracle_search(sh.c, "AND", terms, 0, 64)
        assert set(sh.special) <= {d for d, _, _ in want} and len(sh.special) == 40
        assert {sh.wdf["e1"][d] for d in sh.special} >= {1, 2, 3}
        (hits, hdr), = search_batch(sh.db, [plan(sh.db, Query("AND", terms), 0, 64)])
        assert [(h.docid, h.weight, h.subqs_matched) for h in hits] == want and hdr.matches_exact == oh.matches == sum(n), terms


# ---- the tallies against counts derived from the postings ----

def units_of(db, p):
    kern = C.create_string_buffer(64)
    units = (C.c_uint32 * (4 * 4096))()
    n = _lib.lib().xgm_debug_plan_batch(db._h, C.byref(p), 1, kern, units, 4096)
    assert 0 < n <= 4096, n
    return [(units[4 * i + 1], units[4 * i + 2]) for i in range(n)]


def test_unit_spans(shard):
    """What the planner cut: with XGM_MAX_UNITS_PER_QUERY = 1 / 2 every query here is one unit of 8 stripes / two of 4 — in the one-query call and in the batch."""
    sh = shard
    qs = MIXED_Q + TRAP_Q + TALLY_Q + [["e1", "e2"], ["e1", "e2", "z0"]]
    plans = [plan(sh.db, Query("AND", terms), 0, k) for terms in qs for k in PAGES]
    for p in plans:
        units = units_of(sh.db, p)
        assert sorted(units) == sorted(set(units)) and sum(se - sb for sb, se in units) == N_STRIPES, units
        if UNITS_CAP:
            assert units == SPANS[UNITS_CAP], (UNITS_CAP, units)
    if UNITS_CAP:
        kern = C.create_string_buffer(64)
        units = (C.c_uint32 * (4 * 4096))()
        arr = (type(plans[0]) * len(plans))(*plans)
        n = _lib.lib().xgm_debug_plan_batch(sh.db._h, arr, len(plans), kern, units, 4096)
        assert n == len(plans) * len(SPANS[UNITS_CAP]), n
        assert {(units[4 * i + 1], units[4 * i + 2]) for i in range(n)} == set(SPANS[UNITS_CAP])


def test_planes_are_loaded_once(shard):
    """Bitmap words streamed (xgm_last_batch_traffic [0]): T x W / 32 per stripe in which every term has a container, and the same once more per exact stripe —
    whether the planes were wanted by the new code alone (no threshold yet) or by the class prefilter too (a threshold from earlier stripes of the unit)."""
    sh = shard
    if NO_EXACT or NO_SUM:
        return
    for terms in (["a", "b"], ["a", "b", "c"], ["a", "b", "c", "d"], ["zm", "a", "b"], ["e1", "e2"]):
        for k in (1, 10):
            p = plan(sh.db, Query("AND", terms), 0, k)
            sh.db.set_profiling(2)
            search_batch(sh.db, [p])
            tl = (C.c_uint64 * 10)()
            assert _lib.lib().xgm_last_batch_traffic(sh.db._h, tl, 10) == 0
            sh.db.set_profiling(0)
            n = matches_per_stripe(sh, terms)
            anded = sum(1 for s in range(N_STRIPES) if all(any(d >> SB == s for d in sh.wdf[t]) for t in terms))
            exact = sum(1 for s in range(N_STRIPES) if n[s] >= EXACT_MIN)
            assert anded == 7 + ("a" not in terms) and exact >= 3
            assert tl[0] == len(terms) * (W // 32) * (anded + exact), (terms, k, list(tl), anded, exact)


def summary_bit(sh, t, d):
    """A posting of t with a wdf other than 1 among the 16 slots of d's group."""
    g = d >> (SB - 6)
    return any(sh.wdf[t].get(x, 1) != 1 for x in range(g << (SB - 6), (g + 1) << (SB - 6)))


def dense_counts(sh, terms, units, exact=not NO_EXACT, summary=not NO_SUM):
    """(distinct 64-byte sectors among the lanes that ask, lanes that ask): rounds of 64 consecutive candidates of a unit.  A stripe with >= 48 documents of the
    AND is exact: a term without a posting of wdf 0 is asked iff the document's wdf is >= 2; every other (stripe, term) goes by the summary bit."""
    probes = raw = 0
    cand = sorted(set.intersection(*(set(sh.wdf[t]) for t in terms)))
    per_stripe = matches_per_stripe(sh, terms)
    for sb, se in units:
        mine = [d for d in cand if sb <= d >> SB < se]
        for i in range(0, len(mine), 64):
            rnd = mine[i:i + 64]
            for t in terms:
                def asks(d):
                    if not summary: return True
                    if exact and per_stripe[d >> SB] >= EXACT_MIN and 0 not in sh.wdf[t].values(): return sh.wdf[t][d] >= 2
                    return summary_bit(sh, t, d)
                ask = [d for d in rnd if asks(d)]
                probes += len({d >> 6 for d in ask}); raw += len(ask)
    return probes, raw


def test_tallies_against_the_postings(shard):
    """One crowded stripe of 48 .. 60 matches, at most 64 in the unit: no threshold forms, the prefilter drops nothing, no lane holds more than 8 candidates."""
    sh = shard
    for terms in TALLY_Q:
        p = plan(sh.db, Query("AND", terms), 0, 10)
        units = units_of(sh.db, p)
        sh.db.set_profiling(2)
        search_batch(sh.db, [p])
        tl = (C.c_uint64 * 10)()
        assert _lib.lib().xgm_last_batch_traffic(sh.db._h, tl, 10) == 0
        sh.db.set_profiling(0)
        want = dense_counts(sh, terms, units)
        print("tallies", terms, units, "probes, raw:", (tl[1], tl[8]), "want", want)
        assert (tl[1], tl[8]) == want, (terms, units, list(tl), want)
        assert tl[2] == 0 and tl[3] == 0, list(tl)                   # the dense body: no block decoded
    for terms in TALLY_Q:                                            # the rule removes probes here, or the test shows nothing
        assert dense_counts(sh, terms, [(0, N_STRIPES)], exact=True, summary=True)[1] < dense_counts(sh, terms, [(0, N_STRIPES)], exact=False, summary=True)[1]


# ---- the switches: the same tests in child processes ----

def run_child(env_add, select):
    env = dict(os.environ, **env_add)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", select, "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout, "%r:\n%s\n%s" % (env_add, r.stdout[-3000:], r.stderr[-2000:])


OURS = "conjunctions_vs_oracle or seams or tallies or wdf0_flags"
SWITCHES = [("XGM_NO_EXACT_WDF", OURS), ("XGM_NO_EXACT_WDF,XGM_NO_WDF_SUMMARY", OURS), ("XGM_NO_EXACT_WDF,XGM_NO_NARROW_DOCLEN", OURS),
            ("XGM_NO_EXACT_WDF,XGM_NO_DENSE_BODY", "conjunctions_vs_oracle")]


@pytest.mark.parametrize("switch,select", SWITCHES if not QUICK else SWITCHES[:2])
def test_switches(built, switch, select):
    if NO_EXACT or UNITS_CAP:
        return                                                      # (a child does not start children)
    run_child({name: "1" for name in switch.split(",")}, select)


@pytest.mark.parametrize("cap", ["1", "2"])
def test_units_spanning_stripes(built, cap):
    """Units of 8 and of 4 stripes (the planner's own cut here is one stripe a unit), the path on."""
    if NO_EXACT or UNITS_CAP:
        return
    run_child({"XGM_MAX_UNITS_PER_QUERY": cap}, "unit_spans or planes_are_loaded or " + OURS)
