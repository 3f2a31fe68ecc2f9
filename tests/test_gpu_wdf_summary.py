"""The containers' 64-bit wdf >= 2 summary (xgm_seg_dev::dense_p2, xapiand_amd/csrc/xgm_dense.hip) and its two users: xgm_dense_unit takes wdf = 1 from a
clear summary bit instead of probing the byte, xgm_flat_unit screens by the bitmap (one bit) and fetches the screen's wdf byte only for the survivors whose
summary bit is set.  Hand-made documents on 8 stripes of 1024 (one summary bit covers 16 slots, a bitmap sector 512, a byte sector 64):

  stripe 1   c1's only wdf >= 2 stand at slots 0, 15, 16 and W - 1        stripe 5   c1 all wdf 1, c2 all wdf 2: clear and set in the same lane
  stripe 2   every wdf is 1: rounds in which no lane needs a byte          stripe 6   c1 has no posting: no container, no summary
  stripe 3   c1, c2, c4 all wdf >= 2: every lane needs every byte          stripe 7   crowded (the class prefilter meets the summary)
  stripe 4   c1's wdf >= 2 only in documents no other term indexes: a candidate's bit is set by a neighbour, its byte reads 2

c3 has wdf 1 everywhere (all words 0), c4 a wdf of 254.  Against the oracle: docids, weight bit patterns, exact match counts; the summary words against numpy;
the tallies against counts derived from the postings; everything again with the A/B switches, in child processes.  Also runs under the CPU emulation
(tests/test_emu_wdf_summary.py)."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
from xapiand_amd import Database, Query, _lib
from xapiand_amd.enquire import plan, search_batch, search_batch_replay, search_replay

pytestmark = [pytest.mark.gpu]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = bool(os.environ.get("XGM_EMU_QUICK"))
SB, W, N_STRIPES = 10, 1024, 8
LAST = N_STRIPES * W - 1                   # docids 1 .. 8191: stripe = docid >> 10; containers from df >= 32 x 8 = 256
CONT, LEADS = ("c1", "c2", "c3", "c4", "c5"), ("ledge", "lnone", "lall", "lgap", "lmix")
ORDER = LEADS + ("f1",) + CONT
NO_SUM, NO_BIT = bool(os.environ.get("XGM_NO_WDF_SUMMARY")), bool(os.environ.get("XGM_NO_BIT_SCREEN"))
EDGE_SLOTS = (0, 31, 32, 511, 512, W - 1)
D254 = 77                                  # the document whose wdf of c4 is 254


def make_postings():
    """{term: {docid: wdf}}, document lengths.  Nothing here depends on the code under test."""
    rng = random.Random(0x5D2B17)
    wdf = {t: {} for t in ORDER}
    p = {"c1": 0.45, "c2": 0.55, "c3": 0.65, "c4": 0.80}
    for d in range(1, LAST + 1):
        s, slot = d >> SB, d & (W - 1)
        for t in ("c1", "c2", "c3", "c4"):
            if t == "c1" and s == 6:
                continue
            if rng.random() < (0.9 if s == 7 and t != "c4" else p[t]):
                wdf[t][d] = 1 if t == "c3" or rng.random() < 0.8 else rng.randint(2, 4)
        if rng.random() < 0.04: wdf["c5"][d] = 1 if rng.random() < 0.7 else 2     # a sparse container term: under 48 matches a stripe with anything
        if s == 1 and d in wdf["c1"]: wdf["c1"][d] = 1
        if s == 2:
            for t in CONT:
                if d in wdf[t]: wdf[t][d] = 1
        if s == 3:
            for t in ("c1", "c2", "c4"):
                if d in wdf[t]: wdf[t][d] = 2 + (d % 3)
        if s == 4:
            if slot % 16 == 0:                                     # c1 alone, wdf 3: sets the group's bit, matches no conjunction
                for t in ORDER: wdf[t].pop(d, None)
                wdf["c1"][d] = 3
            elif d in wdf["c1"]: wdf["c1"][d] = 1
        if s == 5:
            if d in wdf["c1"]: wdf["c1"][d] = 1
            if d in wdf["c2"]: wdf["c2"][d] = 2
    for slot, w in ((0, 2), (15, 3), (16, 2), (W - 1, 5)):         # stripe 1: c1's only wdf >= 2
        wdf["c1"][W + slot] = w
    for t in ("c1", "c2", "c4"): wdf[t].setdefault(1, 1)
    wdf["c1"][1] = 2                                               # docid 1: slot 1 of stripe 0
    for t in ("c1", "c2", "c4"): wdf[t].setdefault(D254, 1)
    wdf["c4"][D254] = 254
    for d in range(5, W, 97): wdf["c2"][d] = 0                     # boolean postings (wdf 0: the byte reads 1, not 2 — the summary bit must be set)
    stripe = lambda s: range(max(1, s * W), (s + 1) * W)
    edge = [s * W + slot for s in (1, 3, 5) for slot in EDGE_SLOTS]
    for d in edge:                                                 # lead postings at the sector and word seams, members of every container term
        for t in ("c1", "c2", "c3", "c4"): wdf[t].setdefault(d, 1)
    for d in sorted(set(edge) | set(rng.sample(range(1, LAST + 1), 40))): wdf["ledge"][d] = 1 + d % 2
    for d in rng.sample(stripe(2), 70):                            # nobody survives the screen c1
        wdf["lnone"][d] = 1; wdf["c1"].pop(d, None); wdf["c2"].setdefault(d, 1)
    for d in rng.sample([x for x in stripe(3) if x not in edge], 64):   # a round every lane survives
        wdf["lall"][d] = 2
        for t in ("c1", "c2", "c4"): wdf[t].setdefault(d, 2)
        wdf["c3"].setdefault(d, 1)
    for d in rng.sample(stripe(5), 50) + rng.sample(stripe(6), 50): wdf["lgap"][d] = 1     # stripe 6: the screen c1 has no container
    for d in rng.sample(range(1, LAST + 1), 180): wdf["lmix"].setdefault(d, 1 + d % 3)
    for d in range(4 * W, 5 * W, 16):                              # (stripe 4's lone documents stay lone)
        for t in LEADS: wdf[t].pop(d, None)
    lead_docs = sorted(set().union(*(wdf[t].keys() for t in LEADS)))
    for d in rng.sample(lead_docs, 200): wdf["f1"][d] = 1 + d % 2  # a screen without containers
    post, doclen = {t: [] for t in ORDER}, {}
    for d in range(1, LAST + 1):
        mine = [t for t in ORDER if wdf[t].get(d, 0) > 0]
        toks = [t for t in mine for _ in range(wdf[t][d] - (d % 2))] + ["x%d" % rng.randrange(4) for _ in range(rng.randint(3, 40))]
        rng.shuffle(toks)
        if d % 2: toks = mine + toks                               # every other document: one occurrence of each of its terms side by side (phrases match there)
        doclen[d] = len(toks)
        where = {}
        for pos, t in enumerate(toks, 1): where.setdefault(t, []).append(pos)
        for t, pp in where.items(): post.setdefault(t, []).append((d, len(pp), pp))
        for t in ORDER:
            if wdf[t].get(d) == 0: post[t].append((d, 0, []))      # a boolean posting: indexed, wdf 0, no position
    return post, doclen


class Shard:
    pass


@pytest.fixture(scope="module")
def shard(built, tmp_path_factory):
    post, doclen = make_postings()
    c = H.ManualCorpus(post, doclen)
    sh = Shard()
    sh.c, sh.post = c, post
    sh.wdf = {t: {d: w for d, w, _ in post[t]} for t in ORDER}
    df = {t: len(post[t]) for t in ORDER}
    assert all(df[t] < 32 * N_STRIPES for t in LEADS + ("f1",)) and all(df[t] >= 512 for t in CONT[:4]) and df["c5"] >= 32 * N_STRIPES, df
    assert all(df[t] < df["f1"] for t in LEADS) and df["f1"] < df["c5"] < df["c1"] < df["c2"] < df["c3"] < df["c4"], df
    assert sh.wdf["c4"][D254] == 254 and max(max(v.values()) for v in sh.wdf.values()) == 254 and min(sh.wdf["c2"].values()) == 0
    sh.db = Database(c.build_segment(str(tmp_path_factory.mktemp("wdfsum") / "s.seg"), stripe_bits=SB))
    sh.tid = {}
    for t in ORDER:
        tid, tf = C.c_uint32(), C.c_uint32()
        _lib.check(_lib.lib().xgm_lookup_term(sh.db._h, t.encode(), len(t), C.byref(tid), C.byref(tf), None, None))
        sh.tid[t] = tid.value
    if not any(os.environ.get(v) for v in ("XGM_NO_DENSE", "XGM_DENSE_MIN_AVG")):
        for t in ORDER:                                            # the intended terms got, or did not get, containers
            n = _lib.lib().xgm_debug_read_container(sh.db._h, sh.tid[t], 0, None, 0, None)
            assert (n != 0) == (t in CONT), (t, n)
    yield sh
    sh.db.close()
    c.close()


def want_summary(sh, t, s):
    """None: no container in the stripe.  Bit j: a posting with a wdf other than 1 in slots [16 j, 16 j + 16)."""
    mine = [(d, w) for d, w in sh.wdf[t].items() if d >> SB == s]
    if not mine:
        return None
    word = 0
    for d, w in mine:
        if w != 1: word |= 1 << ((d & (W - 1)) >> (SB - 6))
    return word


def read_summary(sh, t, s):
    out = C.c_uint64(0xDEADBEEFCAFEF00D)
    rc = _lib.lib().xgm_debug_read_wdf_summary(sh.db._h, sh.tid[t], s, C.byref(out))
    assert rc in (0, 1), (t, s, rc, _lib.lib().xgm_last_error())
    assert rc == 1 or out.value == 0xDEADBEEFCAFEF00D, (t, s)        # nothing returned: *out untouched
    return out.value if rc == 1 else None


def test_summary_words_against_numpy(shard):
    sh = shard
    for t in ORDER:
        for s in range(N_STRIPES):
            want = want_summary(sh, t, s) if t in CONT and not NO_SUM else None
            assert read_summary(sh, t, s) == want, (t, s)
    out = C.c_uint64(0)
    assert _lib.lib().xgm_debug_read_wdf_summary(sh.db._h, sh.tid["c1"], N_STRIPES, C.byref(out)) < 0        # stripe out of range
    # what the corpus was built to hold, said once more in plain figures
    assert want_summary(sh, "c1", 1) == (1 << 0) | (1 << 1) | (1 << 63)                          # slots 0 and 15, 16, W - 1
    assert want_summary(sh, "c1", 0) & 1 and sh.wdf["c1"][1] >= 2     # docid 1
    assert want_summary(sh, "c1", 6) is None                          # a stripe without a container
    assert want_summary(sh, "c4", D254 >> SB) >> ((D254 & (W - 1)) >> 4) & 1
    assert all(w == 1 for w in sh.wdf["c3"].values()) and all(want_summary(sh, "c3", s) == 0 for s in range(N_STRIPES))
    assert sh.wdf["c2"][5] == 0 and want_summary(sh, "c2", 0) & 1     # a boolean posting sets its bit
    assert all(want_summary(sh, t, 2) == 0 for t in CONT) and want_summary(sh, "c1", 5) == 0 and bin(want_summary(sh, "c2", 5)).count("1") == 64
    lone = [d for d in range(4 * W, 5 * W, 16)]                       # bits set by postings no query matches
    assert all(sh.wdf["c1"][d] >= 2 and not any(d in sh.wdf[t] for t in ORDER if t != "c1") for d in lone) and want_summary(sh, "c1", 4) == (1 << 64) - 1


def test_summary_switched_off_in_a_child_process(shard):
    if NO_SUM:
        return                                                      # (this IS the child: test_summary_words_against_numpy has looked)
    run_child({"XGM_NO_WDF_SUMMARY": "1"}, "summary_words")


SHAPES = [(0, 1), (0, 10), (0, 64), (3, 7)]
DENSE_Q = [("AND", ["c1", "c2"], 0), ("AND", ["c2", "c4"], 0), ("AND", ["c1", "c2", "c4"], 0), ("AND", ["c1", "c2", "c3"], 0), ("AND", ["c3", "c5"], 0),
           ("AND", ["c1", "c2", "c3", "c4"], 0), ("AND", ["c5", "c1", "c2", "c4"], 0), ("FILTER", ["c2", "c1", "c4"], 1)]
FLAT_Q = [("AND", ["ledge", "c1", "c2"], 0), ("AND", ["ledge", "c1", "c2", "c4"], 0), ("AND", ["lnone", "c1", "c2"], 0), ("AND", ["lall", "c1", "c2"], 0),
          ("AND", ["lall", "c1", "c3", "c4"], 0), ("AND", ["lgap", "c1", "c2"], 0), ("AND", ["lgap", "c1", "c3", "c4"], 0), ("AND", ["lmix", "c5", "c2"], 0),
          ("AND", ["lmix", "f1", "c1"], 0), ("AND", ["lmix", "f1", "c1", "c2"], 0), ("AND", ["ledge", "c1"], 0), ("AND", ["lmix", "f1"], 0),
          ("FILTER", ["lmix", "c1", "c2"], 1), ("FILTER", ["ledge", "c2", "c1", "c4"], 1)]


def conj_cases():
    qs = DENSE_Q + FLAT_Q
    return [(op, terms, nr, first, maxitems) for i, (op, terms, nr) in enumerate(qs) for first, maxitems in (SHAPES if not QUICK else SHAPES[i % 4:][:1])]


def test_conjunctions_vs_oracle(shard):
    """Conjunctions of 2, 3 and 4 container terms (dense body) and led by a long-tail term (flat body): the batch entry point — tallying and plain
    instantiations — and each query alone (cut into other units: the same answer)."""
    sh = shard
    cases = conj_cases()
    plans = [plan(sh.db, Query(op, terms, n_required=nr), first, maxitems) for op, terms, nr, first, maxitems in cases]
    sh.db.set_profiling(2)
    tallied = search_batch(sh.db, plans)
    sh.db.set_profiling(0)
    plain = search_batch(sh.db, plans)
    seen_wdf2 = 0
    for (op, terms, nr, first, maxitems), p, (hits, hdr), (hits0, hdr0) in zip(cases, plans, tallied, plain):
        what = (op, terms, first, maxitems)
        want, oh = H.oracle_search(sh.c, op, terms, first, maxitems, n_required=nr)
        assert [(h.docid, h.weight, h.subqs_matched) for h in hits0] == want, what
        assert [(h.docid, h.weight, h.subqs_matched) for h in hits] == want, what
        assert hdr.matches_exact == oh.matches and hdr0.matches_exact == oh.matches and hdr0.max_possible == oh.max_possible, what
        if want:
            assert hdr0.max_attained == oh.max_attained, what
        (h1, hdr1), = search_batch(sh.db, [p])
        assert [(h.docid, h.weight, h.subqs_matched) for h in h1] == want and hdr1.matches_exact == oh.matches, what
        seen_wdf2 += sum(1 for d, _, _ in want for t in terms if sh.wdf[t][d] >= 2)
        if terms[0] == "lnone":
            assert oh.matches == 0, what                             # the round nobody survives
        if terms[:3] == ["lall", "c1", "c2"]:
            assert oh.matches == 64, what                            # the round every lane survives
        if terms == ["c1", "c2", "c4"]:
            assert oh.matches > 48 * N_STRIPES, what                 # crowded stripes: the class prefilter runs
    assert seen_wdf2 > len(cases), seen_wdf2                         # the pages hold documents whose weight needs a fetched byte


def test_conjunctions_counted_in_the_batch(shard):
    """XGM_REPLAY_BATCH_COUNT (the ALL form lists every match, whatever the threshold says)."""
    sh = shard
    cases = [x for x in conj_cases() if x[3] == 0]
    plans = [plan(sh.db, Query(op, terms, n_required=nr), first, maxitems, check_at_least=first + maxitems) for op, terms, nr, first, maxitems in cases]
    got = search_batch_replay(sh.db, plans, replay=_lib.XGM_REPLAY_BATCH_COUNT)
    for (op, terms, nr, first, maxitems), p, (page, hdr, known) in zip(cases, plans, got):
        what = (op, terms, first, maxitems)
        want, oh = H.oracle_search(sh.c, op, terms, first, maxitems, n_required=nr)
        assert page == want and hdr.matches_exact == oh.matches, (what, hdr.matches_exact, oh.matches)
        _, _, want_known = search_replay(sh.db, p)
        assert known == want_known and known <= oh.matches, (what, known, want_known, oh.matches)


def test_unchanged_paths_phrases_and_frozen(shard):
    sh = shard
    phrases = [["c1", "c2"], ["c1", "c2", "c4"], ["ledge", "c1", "c2"], ["lmix", "f1", "c1"]]
    cases = [(terms, 0, k) for i, terms in enumerate(phrases) for k in ((1, 10) if not QUICK else (10,))]
    plans = [plan(sh.db, Query("PHRASE", terms), first, maxitems) for terms, first, maxitems in cases]
    got = search_batch(sh.db, plans)
    frozen = search_batch_replay(sh.db, [plan(sh.db, Query("PHRASE", terms), first, maxitems, check_at_least=first + maxitems) for terms, first, maxitems in cases])
    n_hits = 0
    for what, (hits, hdr), (page, _, _) in zip(cases, got, frozen):
        terms, first, maxitems = what
        want, oh = H.oracle_search(sh.c, "PHRASE", terms, first, maxitems)
        assert [(h.docid, h.weight, h.subqs_matched) for h in hits] == want, what
        H.check_matches(hdr.matches_exact, oh.matches, len(hits), what)
        ref, _ = H.oracle_search(sh.c, "PHRASE", terms, first, maxitems, reference_select_bug=True)
        assert page == ref, what
        n_hits += len(want)
    assert n_hits >= len(cases), n_hits


# ---- the tallies against counts derived from the postings ----

def units_of(db, p):
    kern = C.create_string_buffer(64)
    units = (C.c_uint32 * (4 * 4096))()
    n = _lib.lib().xgm_debug_plan_batch(db._h, C.byref(p), 1, kern, units, 4096)
    assert 0 < n <= 4096, n
    return [(units[4 * i + 1], units[4 * i + 2]) for i in range(n)]


def sectors(dids, sh_):
    return len({d >> sh_ for d in dids})


def bit_set(sh, t, d):
    w = want_summary(sh, t, d >> SB)
    return bool(w >> ((d & (W - 1)) >> (SB - 6)) & 1)


def dense_counts(sh, terms, units):
    """(distinct byte sectors among the lanes that ask, lanes that ask) of xgm_dense_unit: rounds of 64 consecutive candidates of a unit."""
    probes = raw = 0
    cand = sorted(set.intersection(*(set(sh.wdf[t]) for t in terms)))
    for sb, se in units:
        mine = [d for d in cand if sb <= d >> SB < se]
        for i in range(0, len(mine), 64):
            rnd = mine[i:i + 64]
            for t in terms:
                ask = rnd if NO_SUM else [d for d in rnd if bit_set(sh, t, d)]
                probes += sectors(ask, 6); raw += len(ask)
    return probes, raw


def flat_counts(sh, terms, units):
    """The same of xgm_flat_unit at T = 3, every other term with containers: rounds of 64 lead postings of the unit's docid range; the screen by bit (a
    sector of 512 documents) or by byte; the survivors' screen byte where the summary bit is set; the third term's byte for the survivors."""
    lead, scr, third = terms
    probes = raw = 0
    has_cont = lambda t, d: any(x >> SB == d >> SB for x in sh.wdf[t])
    for sb, se in units:
        mine = sorted(d for d in sh.wdf[lead] if sb <= d >> SB < se)
        for i in range(0, len(mine), 64):
            rnd = mine[i:i + 64]
            ask = [d for d in rnd if has_cont(scr, d)]
            probes += sectors(ask, 6 if NO_BIT else 9); raw += len(ask)
            alive = [d for d in rnd if d in sh.wdf[scr]]
            if not alive:
                continue
            if not NO_BIT:
                ask = alive if NO_SUM else [d for d in alive if bit_set(sh, scr, d)]
                probes += sectors(ask, 6); raw += len(ask)
            ask = [d for d in alive if has_cont(third, d)]
            probes += sectors(ask, 6); raw += len(ask)
    return probes, raw


def test_tallies_against_the_postings(shard):
    """Two fixed queries whose stripes hold fewer than 48 matches (the class prefilter never drops a candidate): what the tallying instantiation counted."""
    sh = shard
    for terms, model in ((["c5", "c2", "c4"], dense_counts), (["ledge", "c1", "c2"], flat_counts)):
        p = plan(sh.db, Query("AND", terms), 0, 10)
        units = units_of(sh.db, p)
        sh.db.set_profiling(2)
        search_batch(sh.db, [p])
        tl = (C.c_uint64 * 10)()
        assert _lib.lib().xgm_last_batch_traffic(sh.db._h, tl, 10) == 0
        sh.db.set_profiling(0)
        want = model(sh, terms, units)
        assert (tl[1], tl[8]) == want, (terms, units, list(tl), want)
        assert tl[2] == 0 and tl[3] == 0, list(tl)                   # a body, not the queue path: no block decoded


# ---- the switches: the same tests in child processes ----

def run_child(env_add, select):
    env = dict(os.environ, **env_add)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", select, "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout, "%r:\n%s\n%s" % (env_add, r.stdout[-3000:], r.stderr[-2000:])


OURS = "conjunctions_vs_oracle or tallies or summary_words"
SWITCHES = [("XGM_NO_WDF_SUMMARY", OURS), ("XGM_NO_BIT_SCREEN", OURS), ("XGM_NO_WDF_SUMMARY,XGM_NO_BIT_SCREEN", OURS),
            ("XGM_NO_WDF_SUMMARY,XGM_NO_NARROW_DOCLEN", OURS), ("XGM_NO_BIT_SCREEN,XGM_NO_NARROW_DOCLEN", OURS),
            ("XGM_NO_DENSE_BODY", "conjunctions_vs_oracle"), ("XGM_NO_FLAT", "conjunctions_vs_oracle")]


@pytest.mark.parametrize("switch,select", SWITCHES if not QUICK else SWITCHES[:3])
def test_switches(built, switch, select):
    if any(os.environ.get(v) for v, _ in SWITCHES[:2] + SWITCHES[5:]):
        return                                                      # (a child does not start children)
    run_child({name: "1" for name in switch.split(",")}, select)
