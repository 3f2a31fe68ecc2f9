"""xgm_flat_unit's staged probes (xapiand_amd/csrc/xgm_flat_body.inc): stage A asks the screen — plan position 1, the other term with the fewest
postings — about the round's 64 lead postings, stage B asks the remaining terms about the survivors only, and the next round's lead postings are
requested one round ahead from an index clamped to the unit's slice.  Hand-made documents on 8 stripes of 1024 put every edge in reach at the
smallest size: lead slices of exactly 64 and 65 postings, a slice that is no multiple of 64, one that ends with the very last entry of the flat
arrays, a round nobody survives and one every lane survives, stripes where the screen (or only a stage-B term) has no container, a screen that is
itself a flat array (binary search), both kinds at T = 4 — against the oracle: docids, weight bit patterns, exact match counts; AND / FILTER,
k = 1 / 10 / 64; the batch and the one-query entry points; XGM_REPLAY_BATCH_COUNT (ALL form); phrases with and without XGM_REPLAY_BATCH_FROZEN (LIST and
PHRASE forms); a launch that mixes the dense body, the flat body and the queue path.  Also runs under the CPU emulation (tests/test_emu_flat_staged.py)."""
import ctypes as C
import os
import random

import pytest

import helpers as H
from xapiand_amd import Database, Query, _lib
from xapiand_amd.enquire import plan, search_batch, search_batch_replay, search_replay

pytestmark = [pytest.mark.gpu]

QUICK = bool(os.environ.get("XGM_EMU_QUICK"))
SB, W, N_STRIPES = 10, 1024, 8
LAST = N_STRIPES * W - 1                   # docids 1 .. 8191: stripe = docid >> 10; containers from df >= 32 x 8 = 256
DENSE, LEADS = ("d1", "d2", "d3"), ("l64", "l65", "lnone", "lgap", "lmix", "zlast")
ORDER = LEADS + ("f1",) + DENSE            # the order the terms of a document stand in where they stand together (phrases match there)
VARIANT = any(os.environ.get(v) for v in ("XGM_NO_FLAT", "XGM_NO_DENSE", "XGM_NO_ANDW", "XGM_NO_AND_KERNEL", "XGM_NO_FLAT_PHRASE", "XGM_NO_POS_PRUNE",
                                          "XGM_NO_PHRASEW", "XGM_NO_DENSE_PHRASE_BODY", "XGM_DENSE_MIN_AVG"))


def make_postings():
    rng = random.Random(0x57A6ED)
    stripe = lambda s: range(max(1, s * W), (s + 1) * W)
    has = {t: set() for t in ORDER}
    for d in range(1, LAST + 1):
        s = d >> SB
        if s != 5 and rng.random() < 0.30: has["d1"].add(d)        # no container of d1 in stripe 5 ...
        if s != 6 and rng.random() < 0.40: has["d2"].add(d)        # ... none of d2 in stripe 6
        if rng.random() < 0.50: has["d3"].add(d)
    has["l64"] = set(rng.sample(stripe(2), 64))                    # a slice of exactly 64, every posting in d1, d2 and d3: every lane survives
    for t in DENSE: has[t] |= has["l64"]
    has["l65"] = set(rng.sample(stripe(3), 65))                    # 64 + 1
    has["lnone"] = set(rng.sample(stripe(4), 70))                  # nobody survives the screen d1; all of them are in d2
    has["d1"] -= has["lnone"]; has["d2"] |= has["lnone"]
    has["lgap"] = set(rng.sample(stripe(5), 50) + rng.sample(stripe(6), 50))
    has["lmix"] = set(rng.sample(range(1, LAST + 1), 180))
    has["zlast"] = set(rng.sample(range(1, LAST), 149)) | {LAST}   # the last term of the dictionary: its slice ends the flat arrays
    lead_docs = sorted(set().union(*(has[t] for t in LEADS)))
    has["f1"] = set(rng.sample(lead_docs, 200))                    # a screen without containers: more postings than any lead, fewer than 256
    post, doclen = {t: [] for t in ORDER}, {}
    for d in range(1, LAST + 1):
        mine = [t for t in ORDER if d in has[t]]
        occ = [t for t in mine for _ in range(rng.randint(1, 3))] + ["x%d" % rng.randrange(4) for _ in range(rng.randint(4, 12))]
        rng.shuffle(occ)
        toks = (mine + occ) if rng.random() < 0.5 else occ         # half of the documents: their terms once more, side by side in ORDER
        doclen[d] = len(toks)
        where = {}
        for p, t in enumerate(toks, 1):
            where.setdefault(t, []).append(p)
        for t, pp in where.items():
            post.setdefault(t, []).append((d, len(pp), pp))
    return post, doclen


@pytest.fixture(scope="module")
def shard(built, tmp_path_factory):
    post, doclen = make_postings()
    c = H.ManualCorpus(post, doclen)
    df = {t: len(post[t]) for t in ORDER}
    assert all(df[t] < 32 * N_STRIPES for t in LEADS + ("f1",)) and all(df[t] >= 2 * 32 * N_STRIPES for t in DENSE), df
    assert all(df[t] < df["f1"] for t in LEADS) and df["l64"] == 64 and df["l65"] == 65 and c.terms()[-1] == b"zlast", df
    db = Database(c.build_segment(str(tmp_path_factory.mktemp("staged") / "s.seg"), stripe_bits=SB))
    yield c, db
    db.close()
    c.close()


CONJ = [("AND", ["l65", "d1"], 0), ("AND", ["lmix", "f1"], 0), ("AND", ["zlast", "d3"], 0),
        ("AND", ["l64", "d1", "d2"], 0), ("AND", ["l65", "d1", "d2"], 0), ("AND", ["lnone", "d1", "d2"], 0), ("AND", ["lgap", "d1", "d2"], 0),
        ("AND", ["lmix", "f1", "d1"], 0), ("AND", ["zlast", "f1", "d2"], 0), ("AND", ["zlast", "d1", "d3"], 0),
        ("AND", ["lmix", "f1", "d1", "d2"], 0), ("AND", ["l64", "d1", "d2", "d3"], 0), ("AND", ["zlast", "f1", "d2", "d3"], 0), ("AND", ["lgap", "d1", "d2", "d3"], 0),
        ("FILTER", ["lmix", "d1", "d2"], 1), ("FILTER", ["zlast", "f1", "d2"], 2), ("FILTER", ["l64", "d2", "d1", "d3"], 2)]
PHRASES = [["l65", "d1"], ["lmix", "d1"], ["lmix", "f1", "d1"], ["zlast", "d1", "d3"], ["l64", "d1", "d2"], ["lgap", "d2", "d3"], ["zlast", "f1"], ["lnone", "d2", "d3"]]
SHAPES = [(0, 1), (0, 10), (0, 64), (3, 7)]


def conj_cases():
    return [(op, terms, nr, first, maxitems) for i, (op, terms, nr) in enumerate(CONJ) for first, maxitems in (SHAPES if not QUICK else SHAPES[i % 4:][:1])]


def test_staged_conjunctions_vs_oracle(shard):
    """AND of 2 / 3 / 4 terms and FILTER, pages of 1 / 10 / 64 and one inside the match: the batch entry point with the tallying instantiation, then each
    query alone (latency mode cuts it into many units: other slices, the same answer)."""
    c, db = shard
    cases = conj_cases()
    plans = [plan(db, Query(op, terms, n_required=nr), first, maxitems) for op, terms, nr, first, maxitems in cases]
    db.set_profiling(2)
    got = search_batch(db, plans)
    tl = (C.c_uint64 * 10)()
    assert _lib.lib().xgm_last_batch_traffic(db._h, tl, 10) == 0
    db.set_profiling(0)
    plain = search_batch(db, plans)
    n_matching = 0
    for (op, terms, nr, first, maxitems), p, (hits, hdr), (hits0, hdr0) in zip(cases, plans, got, plain):
        what = (op, terms, first, maxitems)
        want, oh = H.oracle_search(c, op, terms, first, maxitems, n_required=nr)
        assert [(h.docid, h.weight, h.subqs_matched) for h in hits] == want, what
        assert [(h.docid, h.weight, h.subqs_matched) for h in hits0] == want, what
        assert hdr.matches_exact == oh.matches and hdr0.matches_exact == oh.matches and hdr.max_possible == oh.max_possible, what
        if want:
            assert hdr.max_attained == oh.max_attained, what
        (h1, hdr1), = search_batch(db, [p])
        assert [(h.docid, h.weight, h.subqs_matched) for h in h1] == want and hdr1.matches_exact == oh.matches, what
        n_matching += oh.matches > 0
        if terms[0] == "lnone":
            assert oh.matches == 0, what                     # (the round nobody survives)
        if terms[:3] == ["l64", "d1", "d2"]:
            assert oh.matches == 64, what                    # (the round every lane survives)
    assert n_matching >= len(cases) * 2 // 3, n_matching
    if not VARIANT:
        assert tl[2] == 0 and tl[3] == 0 and tl[5] > 0, list(tl)      # every query took the flat body: no block decoded, flat words streamed


def test_staged_conjunctions_counted_in_the_batch(shard):
    """The same queries with XGM_REPLAY_BATCH_COUNT (the ALL form lists every match): the oracle's page and exact match count; known_matching_docs — which
    the oracle does not restate — equal to the one-query replay's and within the match."""
    c, db = shard
    cases = [x for x in conj_cases() if x[3] == 0]
    plans = [plan(db, Query(op, terms, n_required=nr), first, maxitems, check_at_least=first + maxitems) for op, terms, nr, first, maxitems in cases]
    got = search_batch_replay(db, plans, replay=_lib.XGM_REPLAY_BATCH_COUNT)
    for (op, terms, nr, first, maxitems), p, (page, hdr, known) in zip(cases, plans, got):
        what = (op, terms, first, maxitems)
        want, oh = H.oracle_search(c, op, terms, first, maxitems, n_required=nr)
        assert page == want and hdr.matches_exact == oh.matches, (what, hdr.matches_exact, oh.matches)
        _, _, want_known = search_replay(db, p)
        assert known == want_known and known <= oh.matches, (what, known, want_known, oh.matches)


def test_staged_phrases_vs_oracle(shard):
    """Phrases of 2 - 3 terms led by a long-tail term: the staged loads also carry where the flat terms' positions start.  Without replay bits (PHRASE form)
    against the oracle; with XGM_REPLAY_BATCH_FROZEN (LIST form) against the oracle in the reference's mode."""
    c, db = shard
    cases = [(terms, first, maxitems) for i, terms in enumerate(PHRASES) for first, maxitems in (SHAPES[:3] if not QUICK else SHAPES[i % 3:][:1])]
    plans = [plan(db, Query("PHRASE", terms), first, maxitems) for terms, first, maxitems in cases]
    got = search_batch(db, plans)
    frozen = search_batch_replay(db, [plan(db, Query("PHRASE", terms), first, maxitems, check_at_least=first + maxitems) for terms, first, maxitems in cases])
    n_hits = 0
    for what, p, (hits, hdr), (page, fhdr, _) in zip(cases, plans, got, frozen):
        terms, first, maxitems = what
        want, oh = H.oracle_search(c, "PHRASE", terms, first, maxitems)
        assert [(h.docid, h.weight, h.subqs_matched) for h in hits] == want, what
        H.check_matches(hdr.matches_exact, oh.matches, len(hits), what)
        (h1, hdr1), = search_batch(db, [p])
        assert [(h.docid, h.weight, h.subqs_matched) for h in h1] == want, what
        ref, _ = H.oracle_search(c, "PHRASE", terms, first, maxitems, reference_select_bug=True)
        assert page == ref, what
        n_hits += len(want)
    assert n_hits >= 3 * len(cases), n_hits


def test_dense_flat_and_queue_path_share_a_launch(shard):
    c, db = shard
    cases = [(["d1", "d2", "d3"], 10), (["lmix", "f1", "d1"], 10), (["d1", "d2", "d3"], 100), (["lmix", "f1", "d1", "d2", "d3"], 10), (["zlast", "d1", "d3"], 64),
             (["lgap", "d1", "d2"], 100), (["d2", "d3"], 1)]
    plans = [plan(db, Query("AND", terms), 0, k) for terms, k in cases]
    for (terms, k), (hits, hdr) in zip(cases, search_batch(db, plans)):
        want, oh = H.oracle_search(c, "AND", terms, 0, k)
        assert [(h.docid, h.weight, h.subqs_matched) for h in hits] == want and hdr.matches_exact == oh.matches, (terms, k)
