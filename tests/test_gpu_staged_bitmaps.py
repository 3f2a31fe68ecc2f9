"""xgm_dense_unit's two-stage bitmap loads (plain conjunctions): the bitmaps of plan terms 2 and 3 are asked for only by the lanes whose own 128 documents hold
a bit of terms 0 AND 1, a term index >= T is not loaded at all, and the loads run one stage further ahead — stage 2 of the next qualifying stripe and stage 1 of
the one after it are in flight while a stripe is enumerated.  Hand-made documents on 8 stripes of 1024: 8 lanes hold words, a bitmap is two 64-byte sectors.
The planner cuts so small a shard into units of ONE stripe, so everything also runs in child processes with XGM_MAX_UNITS_PER_QUERY=1 (one unit of all 8
stripes) and =2 (two of 4), the spans asserted through xgm_debug_plan_batch.  p < q < r < s < z in df, so `p q ...` is planned in that order:

  stripe 0   crowded, > 256 documents of `p q r s`: the ring refills mid-stripe       stripe 4   p AND q only at slots 0, 31, 32, 127: lane 0 alone asks
             while stripes 1 and 2 are in flight; the exact-wdf planes                stripe 5   p AND q only at slots 128 and W - 1: lanes 1 and 7
  stripe 1   every term has a container, p AND q is empty: stage 2 asks nothing       stripe 6   lane 2: p q s without r; lane 3: p q r without s; lane 5: all four
  stripe 2   crowded; with a threshold from stripe 0, the class prefilter             stripe 7   crowded
  stripe 3   r has no posting: no container, skipped by all_mask at T >= 3

u1 lives in stripes 2 and 6 only, u2 in 0, 2, 5, 7: with them as the rarest term a unit holds exactly 1 or 2 qualifying stripes, others skipped in between;
`p q r` gives a unit of stripes 0..3 exactly 3.  z: every posting boolean (wdf 0); one wdf of 254 (r) in a document of the first page.  One further shard at
stripe_bits = 13 (3 stripes, sparse terms): all 64 lanes hold words, a bitmap is 16 sectors.
Against the oracle at every rank: docid, weight bit pattern, subqs_matched, match count, maxima; the tallies against counts derived from the postings; the
switches in child processes.  Also runs under the CPU emulation (tests/test_emu_staged_bitmaps.py)."""
import ctypes as C
import os
import random
import subprocess
import sys

import pytest

import helpers as H
from xapiand_amd import Database, Query, _lib
from xapiand_amd.enquire import plan, search_batch, search_batch_replay

pytestmark = [pytest.mark.gpu]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SB, W, N_STRIPES = 10, 1024, 8
LAST = N_STRIPES * W - 1
ORDER = ("u2", "u1", "p", "q", "r", "s", "z")                       # ascending df (asserted): the planner's order
MAIN = ("p", "q", "r", "s")
CROWDED, EMPTY01, NO_R, LANE0, LASTLANE, MIXED = (0, 2, 7), 1, 3, 4, 5, 6
LANE0_SLOTS, LAST_SLOTS = (0, 31, 32, 127), (128, W - 1)
EXACT_MIN = 48                             # XGM_DENSE_EXACT_MIN's default
NO_STAGED, NO_EXACT, NO_SUM = (bool(os.environ.get(n)) for n in ("XGM_NO_STAGED_BITMAPS", "XGM_NO_EXACT_WDF", "XGM_NO_WDF_SUMMARY"))
UNITS_CAP = os.environ.get("XGM_MAX_UNITS_PER_QUERY")                # set in the child processes of test_units_spanning_stripes
SPANS = {"1": [(0, 8)], "2": [(0, 4), (4, 8)]}
D254 = 40                                  # a short document of stripe 0 that holds everything: r's wdf there is 254
SB13, W13, N13 = 13, 8192, 3
ORDER13 = ("a", "b", "c", "d")


def draw_wdf(rng):
    return 1 if rng.random() < 0.6 else rng.randint(2, 4)


def make_postings():
    """{term: {docid: wdf}}, document lengths.  Nothing here depends on the code under test."""
    rng = random.Random(0x57A6ED)
    wdf = {t: {} for t in ORDER}
    prob = {"p": 0.70, "q": 0.75, "r": 0.80, "s": 0.85}

    def put(t, d, w=None):
        wdf[t][d] = 0 if t == "z" else (draw_wdf(rng) if w is None else w)

    for s in range(N_STRIPES):
        base = s * W
        docs = [d for d in range(base, base + W) if d >= 1]
        for d in docs:                                             # z: boolean, nearly everywhere; r and s: frequent everywhere but r's stripe 3
            if rng.random() < 0.9: put("z", d)
            if s != NO_R and rng.random() < prob["r"]: put("r", d)
            if rng.random() < prob["s"]: put("s", d)
        if s in CROWDED:
            for d in docs:
                if rng.random() < prob["p"]: put("p", d)
                if rng.random() < prob["q"]: put("q", d)
        elif s == EMPTY01:                                         # p in lanes 0..3, q in lanes 4..7: containers for both, nothing in common
            for d in docs:
                if rng.random() < 0.5: put("p" if (d & (W - 1)) < W // 2 else "q", d)
        elif s == NO_R:
            for d in docs:
                if rng.random() < 0.2: put("p", d)
                if rng.random() < 0.2: put("q", d)
        else:                                                      # stripes 4, 5, 6: p on even slots, q on odd ones — apart from the documents set below
            for d in docs:
                if rng.random() < 0.4: put("q" if d & 1 else "p", d)
    for x in LANE0_SLOTS:
        for t in MAIN + ("z",): put(t, LANE0 * W + x)
    for x in LAST_SLOTS:
        for t in MAIN + ("z", "u2"): put(t, LASTLANE * W + x)
    lane = lambda l: range(MIXED * W + 128 * l, MIXED * W + 128 * l + 128)
    for l, absent in ((2, "r"), (3, "s"), (5, None)):
        for d in rng.sample(list(lane(l)), 10):
            for t in MAIN + ("z", "u1"):
                if t == absent: wdf[t].pop(d, None)
                else: put(t, d)
    for s in (2, 6):                                               # u1, u2: in half of the lanes only, so that they mask the others
        for d in range(s * W, (s + 1) * W):
            if ((d & (W - 1)) >> 7) in (0, 2, 3, 5) and rng.random() < 0.6: put("u1", d)
    for s in (0, 2, 5, 7):
        for d in range(max(1, s * W), (s + 1) * W):
            if ((d & (W - 1)) >> 7) in (1, 3, 6, 7) and rng.random() < 0.2: put("u2", d)
    for t in MAIN + ("z", "u2"): put(t, D254, 4)
    wdf["r"][D254] = 254
    wdf["p"][LANE0 * W] = 2; wdf["q"][LANE0 * W + 31] = 3; wdf["r"][LANE0 * W + 32] = 1; wdf["s"][LANE0 * W + 127] = 4
    wdf["p"][LASTLANE * W + 128] = 3; wdf["q"][LASTLANE * W + W - 1] = 2
    post, doclen = {t: sorted(wdf[t].items()) for t in ORDER}, {}
    for d in range(1, LAST + 1):
        doclen[d] = sum(wdf[t].get(d, 0) for t in ORDER) + rng.randint(3, 60)
    doclen[D254] = 8                                               # (short, so that it ranks first: the weight formula does not ask the length to cover the wdf)
    return wdf, post, doclen


def make_postings13():
    rng = random.Random(0x13B175)
    prob = {"a": 0.05, "b": 0.06, "c": 0.30, "d": 0.40}
    wdf = {t: {} for t in ORDER13}
    last = N13 * W13 - 1
    for d in range(1, last + 1):
        for t in ORDER13:
            if rng.random() < prob[t]: wdf[t][d] = draw_wdf(rng)
    for d in (1, W13 - 1, W13, W13 + 127, W13 + 128, 2 * W13 + W13 - 1):     # the seams of lanes and stripes: members of everything
        for t in ORDER13: wdf[t][d] = draw_wdf(rng)
    for l in (5, 40):                                              # lanes of stripe 2 with `a b` and without c resp. d
        for d in range(2 * W13 + 128 * l, 2 * W13 + 128 * l + 128):
            wdf["c" if l == 5 else "d"].pop(d, None)
        for d in rng.sample(range(2 * W13 + 128 * l, 2 * W13 + 128 * l + 128), 3):
            wdf["a"][d] = wdf["b"][d] = 1
    post = {t: sorted(wdf[t].items()) for t in ORDER13}
    doclen = {d: sum(wdf[t].get(d, 0) for t in ORDER13) + rng.randint(3, 60) for d in range(1, last + 1)}
    return wdf, post, doclen


class Shard:
    pass


def open_shard(built, path, wdf, post, doclen, order, sb):
    sh = Shard()
    sh.c, sh.wdf, sh.sb, sh.w = H.ManualCorpus(post, doclen, positions=False), wdf, sb, 1 << sb
    sh.n_stripes = (max(doclen) >> sb) + 1
    sh.df = {t: len(post[t]) for t in order}
    assert all(sh.df[t] >= 32 * sh.n_stripes for t in order), sh.df                     # every term has probe containers
    assert all(sh.df[x] < sh.df[y] for x, y in zip(order, order[1:])), sh.df            # ... and the plan order is the order written here
    sh.db = Database(sh.c.build_segment(path, stripe_bits=sb))
    return sh


@pytest.fixture(scope="module")
def shard(built, tmp_path_factory):
    sh = open_shard(built, str(tmp_path_factory.mktemp("staged") / "s.seg"), *make_postings(), ORDER, SB)
    yield sh
    sh.db.close()
    sh.c.close()


@pytest.fixture(scope="module")
def shard13(built, tmp_path_factory):
    sh = open_shard(built, str(tmp_path_factory.mktemp("staged13") / "s.seg"), *make_postings13(), ORDER13, SB13)
    yield sh
    sh.db.close()
    sh.c.close()


def planned(sh, terms):
    return sorted(terms, key=lambda t: sh.df[t])


def docs_of(sh, terms):
    return set.intersection(*(set(sh.wdf[t]) for t in terms))


def per_stripe(sh, terms):
    docs = docs_of(sh, terms)
    return [sum(1 for d in docs if d >> sh.sb == s) for s in range(sh.n_stripes)]


def anded_stripes(sh, terms):
    """Stripes in which every term has a posting, hence a container: the stripes a unit ANDs."""
    return [s for s in range(sh.n_stripes) if all(any(d >> sh.sb == s for d in sh.wdf[t]) for t in terms)]


def masked_lanes(sh, terms, s):
    """Lanes that hold words of stripe s (128 documents each) without a document of plan terms 0 AND 1."""
    t0, t1 = planned(sh, terms)[:2]
    live = {(d & (sh.w - 1)) >> 7 for d in docs_of(sh, [t0, t1]) if d >> sh.sb == s}
    return min(64, sh.w // 128) - len(live)


def skipped_words(sh, terms):
    return sum(4 * (len(terms) - 2) * masked_lanes(sh, terms, s) for s in anded_stripes(sh, terms))


Q2 = [["p", "q"], ["u1", "p"], ["r", "s"]]
Q3 = [["p", "q", "r"], ["u1", "p", "q"], ["u2", "p", "q"], ["q", "r", "s"], ["p", "q", "z"]]
Q4 = [["p", "q", "r", "s"], ["u2", "p", "q", "r"], ["p", "q", "r", "z"]]
QUERIES = Q2 + Q3 + Q4
PAGES = (1, 10)
QUERIES13 = [["a", "b"], ["a", "b", "c"], ["b", "c", "d"], ["a", "b", "c", "d"]]


def test_the_corpus_holds_what_the_cases_need(shard):
    sh = shard
    wdf, lane_of = sh.wdf, lambda d: (d & (W - 1)) >> 7
    n4, n3 = per_stripe(sh, MAIN), per_stripe(sh, ["p", "q", "r"])
    # every term has a container in stripe 1, the AND of the two rarest is empty there, and the stripes on both sides are crowded
    assert EMPTY01 in anded_stripes(sh, MAIN) and per_stripe(sh, ["p", "q"])[EMPTY01] == 0 and masked_lanes(sh, MAIN, EMPTY01) == 8
    assert n4[0] >= EXACT_MIN and n4[2] >= EXACT_MIN and n3[0] >= EXACT_MIN and n3[2] >= EXACT_MIN
    # r has no container in stripe 3, next to staged ones
    assert anded_stripes(sh, MAIN) == [0, 1, 2, 4, 5, 6, 7] == anded_stripes(sh, ["p", "q", "r"]) and anded_stripes(sh, ["p", "q"]) == list(range(8))
    # units with exactly 1, 2 and 3 qualifying stripes (a pipeline shorter than its depth), stripes skipped in between
    assert anded_stripes(sh, ["u1", "p", "q"]) == [2, 6] and anded_stripes(sh, ["u2", "p", "q"]) == [0, 2, 5, 7] == anded_stripes(sh, ["u2", "p", "q", "r"])
    assert [s for s in anded_stripes(sh, ["p", "q", "r"]) if s < 4] == [0, 1, 2]
    # candidates in lane 0 alone / in the last lane and at slot 128
    assert sorted(d - LANE0 * W for d in docs_of(sh, ["p", "q"]) if d >> SB == LANE0) == list(LANE0_SLOTS) and n4[LANE0] == 4 and masked_lanes(sh, MAIN, LANE0) == 7
    assert sorted(d - LASTLANE * W for d in docs_of(sh, ["p", "q"]) if d >> SB == LASTLANE) == list(LAST_SLOTS) and n4[LASTLANE] == 2 and masked_lanes(sh, MAIN, LASTLANE) == 6
    # T = 4: a lane where a01 & t2 is empty and t3 is not, the reverse, and a lane with candidates
    a01 = [d for d in docs_of(sh, ["p", "q"]) if d >> SB == MIXED]
    assert {lane_of(d) for d in a01} == {2, 3, 5}
    assert not any(d in wdf["r"] for d in a01 if lane_of(d) == 2) and all(d in wdf["s"] for d in a01 if lane_of(d) == 2)
    assert all(d in wdf["r"] for d in a01 if lane_of(d) == 3) and not any(d in wdf["s"] for d in a01 if lane_of(d) == 3)
    assert n4[MIXED] == 10 == sum(1 for d in a01 if lane_of(d) == 5)
    # more than 256 candidates in the first stripe of a unit, two further qualifying stripes behind it
    assert n4[0] > 256 and n3[0] > 256 and per_stripe(sh, ["p", "q"])[0] > 256
    # a boolean term, a wdf of 254 in a document that matches
    assert set(wdf["z"].values()) == {0} and wdf["r"][D254] == 254 and D254 in docs_of(sh, MAIN) and max(max(v.values()) for v in wdf.values()) == 254
    # the staged loads skip something in every query of three and four terms, and nothing can be skipped at two
    assert all(skipped_words(sh, terms) > 0 for terms in Q3 + Q4) and all(skipped_words(sh, terms) == 0 for terms in Q2)


def check_vs_oracle(sh, queries):
    cs = [(terms, k) for terms in queries for k in PAGES]
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


def test_conjunctions_vs_oracle(shard):
    """Conjunctions of 2, 3 and 4 terms, k = 1 and 10, at every rank: the batch call — tallying and plain instantiations — and each query alone."""
    check_vs_oracle(shard, QUERIES)
    want, _ = H.oracle_search(shard.c, "AND", list(MAIN), 0, 10)
    assert D254 in {d for d, _, _ in want}                          # the wdf of 254 is weighed on the first page


def test_all_64_lanes_vs_oracle(shard13):
    """stripe_bits = 13: every lane holds words, 16 sectors a bitmap, sparse rarest terms — most lanes are masked."""
    sh = shard13
    assert all(0 < masked_lanes(sh, ["a", "b"], s) < 64 for s in range(N13))
    for l, gone in ((5, "c"), (40, "d")):
        mine = [d for d in docs_of(sh, ["a", "b"]) if d >> SB13 == 2 and (d & (W13 - 1)) >> 7 == l]
        assert mine and not any(d in sh.wdf[gone] for d in mine)
    check_vs_oracle(sh, QUERIES13)


def test_counted_in_the_batch(shard):
    """The ALL form (XGM_REPLAY_BATCH_COUNT lists every match, whatever the threshold says) takes the same staged loads."""
    sh = shard
    for terms in (["p", "q", "r"], ["p", "q", "r", "s"]):
        (page, hdr, known), = search_batch_replay(sh.db, [plan(sh.db, Query("AND", terms), 0, 10, check_at_least=10)], replay=_lib.XGM_REPLAY_BATCH_COUNT)
        want, oh = H.oracle_search(sh.c, "AND", terms, 0, 10)
        assert page == want and hdr.matches_exact == oh.matches == len(docs_of(sh, terms)), (terms, hdr.matches_exact, oh.matches)


# ---- the tallies against counts derived from the postings ----

def units_of(db, p):
    kern = C.create_string_buffer(64)
    units = (C.c_uint32 * (4 * 4096))()
    n = _lib.lib().xgm_debug_plan_batch(db._h, C.byref(p), 1, kern, units, 4096)
    assert 0 < n <= 4096, n
    return [(units[4 * i + 1], units[4 * i + 2]) for i in range(n)]


def test_unit_spans(shard):
    """What the planner cut: with XGM_MAX_UNITS_PER_QUERY = 1 / 2 every query here is one unit of 8 stripes / two of 4."""
    sh = shard
    for terms in QUERIES:
        for k in PAGES:
            units = units_of(sh.db, plan(sh.db, Query("AND", terms), 0, k))
            assert sorted(units) == sorted(set(units)) and sum(se - sb for sb, se in units) == N_STRIPES, units
            if UNITS_CAP:
                assert units == SPANS[UNITS_CAP], (UNITS_CAP, units)


def tallies(sh, terms, k):
    p = plan(sh.db, Query("AND", terms), 0, k)
    sh.db.set_profiling(2)
    search_batch(sh.db, [p])
    tl, skipped = (C.c_uint64 * 10)(), C.c_uint64(1 << 40)
    assert _lib.lib().xgm_last_batch_traffic(sh.db._h, tl, 10) == 0
    assert _lib.lib().xgm_last_batch_bitmap_skipped(sh.db._h, C.byref(skipped)) == 0
    sh.db.set_profiling(0)
    return list(tl), skipped.value


def check_tallies(sh, queries):
    for terms in queries:
        for k in PAGES:
            tl, skipped = tallies(sh, terms, k)
            anded = anded_stripes(sh, terms)
            want = 0 if NO_STAGED else skipped_words(sh, terms)
            print("tallies", terms, k, "bitmap words", tl[0], "skipped", skipped, "want", want)
            assert skipped == want, (terms, k, skipped, want, [masked_lanes(sh, terms, s) for s in anded])
            if len(terms) == 2:
                assert skipped == 0
            if not (NO_EXACT or NO_SUM):                            # the words the ANDs are made of keep their count: T x W / 32 per ANDed stripe, once more per exact stripe
                exact = sum(1 for s, n in enumerate(per_stripe(sh, terms)) if n >= EXACT_MIN)
                assert tl[0] == len(terms) * (sh.w // 32) * (len(anded) + exact), (terms, k, tl, anded, exact)


def test_tallies_against_the_postings(shard):
    """xgm_last_batch_traffic()[0] keeps its value; the words NOT asked for are 4 per masked lane and term >= 2 of every ANDed stripe: 0 at T = 2, 0 with the switch."""
    check_tallies(shard, QUERIES)


def test_tallies_all_64_lanes(shard13):
    check_tallies(shard13, QUERIES13)


def test_skipped_needs_a_tallied_batch(shard):
    """No index, and a last batch that did not tally (its headers' c_pad[0] may hold anything): an error, not a sum over the slots of an earlier batch."""
    sh = shard
    out = C.c_uint64(0)
    assert _lib.lib().xgm_last_batch_bitmap_skipped(None, C.byref(out)) < 0
    assert tallies(sh, ["p", "q", "r"], 10)[1] > 0 or NO_STAGED
    search_batch(sh.db, [plan(sh.db, Query("OR", ["p", "q"]), 0, 10)])
    assert _lib.lib().xgm_last_batch_bitmap_skipped(sh.db._h, C.byref(out)) < 0


# ---- the switches and the longer units: the same tests in child processes ----

def run_child(env_add, select):
    env = dict(os.environ, **env_add)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", select, "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout, "%r:\n%s\n%s" % (env_add, r.stdout[-3000:], r.stderr[-2000:])


OURS = "vs_oracle or counted_in_the_batch or tallies"
SWITCHES = ["XGM_NO_STAGED_BITMAPS", "XGM_NO_STAGED_BITMAPS,XGM_NO_EXACT_WDF", "XGM_NO_STAGED_BITMAPS,XGM_NO_WDF_SUMMARY", "XGM_NO_EXACT_WDF", "XGM_NO_WDF_SUMMARY"]
IN_CHILD = NO_STAGED or NO_EXACT or NO_SUM or bool(UNITS_CAP)


@pytest.mark.parametrize("switch", SWITCHES)
def test_switches(built, switch):
    if IN_CHILD:
        pytest.skip("a child does not start children")             # (never selected there: run_child's -k names OURS)
    run_child({name: "1" for name in switch.split(",")}, OURS)


@pytest.mark.parametrize("cap,switch", [("1", ""), ("2", ""), ("1", "XGM_NO_STAGED_BITMAPS"), ("2", "XGM_NO_STAGED_BITMAPS")])
def test_units_spanning_stripes(built, cap, switch):
    """Units of 8 and of 4 stripes (the planner's own cut here is one stripe a unit): the pipeline at its full depth, its prologue and its end."""
    if IN_CHILD:
        pytest.skip("a child does not start children")
    run_child(dict({"XGM_MAX_UNITS_PER_QUERY": cap}, **({switch: "1"} if switch else {})), "unit_spans or " + OURS)
