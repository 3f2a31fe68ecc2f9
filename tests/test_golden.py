"""CPU-only: the CPU oracle reproduces the committed golden vectors that the real reference
generated (tests/golden/make_golden.py) — docid at every rank identical, weights bit-identical."""
import glob
import json
import os

import pytest

import helpers as H

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "*.json")))

_cache = {}


def shards_for(fx):
    if "coloc" in fx:                      # hand-made documents with several terms per position (NEAR's duplicate-position step)
        key = ("coloc", fx["coloc"]["seed"], fx["coloc"]["n_docs"])
        if key not in _cache:
            _cache[key] = [H.ManualCorpus(*H.coloc_postings(fx["coloc"]["seed"], fx["coloc"]["n_docs"]))]
        return _cache[key]
    if "tree_edges" in fx:                 # the crafted corpus of the nested-query edges (helpers.tree_edge_postings), deleted documents and all
        key = ("tree_edges", fx["tree_edges"]["lastdocid"])
        if key not in _cache:
            assert fx["tree_edges"]["lastdocid"] == H.TREE_EDGE_LASTDOCID
            _cache[key] = [H.ManualCorpus(*H.tree_edge_postings())]
        return _cache[key]
    if "positional_edges" in fx:           # the crafted corpus of the positional filter's edges (helpers.positional_edge_postings)
        key = ("positional_edges", fx["positional_edges"]["lastdocid"], fx["positional_edges"]["seed"])
        if key not in _cache:
            assert key[1:] == (H.POS_EDGE_LASTDOCID, H.POS_EDGE_SEED)
            _cache[key] = [H.ManualCorpus(*H.positional_edge_postings())]
        return _cache[key]
    c = fx["corpus"]
    key = (c["seed"], c["n_docs"], c["vocab"], fx["n_shards"])
    if key not in _cache:
        _cache[key] = [H.Corpus(c["n_docs"], c["vocab"], seed=c["seed"], len_lo=c["len_lo"], len_hi=c["len_hi"],
                                n_shards=fx["n_shards"], shard=s) for s in range(fx["n_shards"])]
    return _cache[key]


def expected(r):
    return [(d, float.fromhex(w)) for d, w, _ in r["hits"]]


def hits_digest(rows, pct):
    """tests/golden/make_golden.py::hits_digest over the oracle's rows: a long page is recorded as its length and this."""
    import hashlib
    return hashlib.sha256("".join("%d %s %d\n" % (d, w.hex(), p) for (d, w, _), p in zip(rows, pct)).encode()).hexdigest()


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_oracle_matches_golden(path):
    fx = json.load(open(path))
    shards = shards_for(fx)
    assert fx["results"]
    for r in fx["results"]:
        q = r["query"]
        if r.get("reference_crashed"):         # recorded without an answer (positional_edges: at most three, named in DESIGN.md)
            continue
        if q["op"] == "RPN":
            rows, hdr, total_subqs = H.oracle_search_tree(shards[0], H.tree_from_json(q["tree"]), q["first"], q["maxitems"])
            page = rows[q["first"]:]
            got = [(d, w) for d, w, _ in page]
            assert hdr.max_possible == float.fromhex(r["max_possible"]), q
            # the best weight of the whole match and the percentages: matched / total weighted subqueries of the best document
            pct = H.tree_percentages(page, hdr, total_subqs) if rows else []
            if rows:
                assert hdr.max_attained == float.fromhex(r["max_attained"]), q
            if "hits" not in r:                # a long page: its length and digest
                assert (len(page), hits_digest(page, pct)) == (r["n_hits"], r["hits_sha256"]), q
                continue
            assert pct == [p for _, _, p in r["hits"]], q
        elif q.get("spy") is not None:
            total, counts = H.oracle_spy(shards[0], q["op"], q["terms"], q["spy"], n_required=q.get("n_required", 0))
            assert (total, [[v.hex(), n] for v, n in counts]) == (r["spy_total"], r["spy"]), q
            continue
        elif q.get("sort"):
            mode, slot, rev = q["sort"]
            hits, hdr = H.oracle_search_sorted(shards[0], q["op"], q["terms"], q["first"], q["maxitems"], mode, slot, rev, n_required=q.get("n_required", 0))
            got = [(d, w) for d, w, _, _ in hits[q["first"]:]]
            assert [k.hex() for _, _, _, k in hits[q["first"]:]] == r["sort_keys"], q
            assert hdr.max_attained == float.fromhex(r["max_attained"]), q
        elif fx["n_shards"] == 1:
            # (co-located NEAR: the reference's answers carry its history dependence and its stale weights — the oracle's reference mode)
            hits, hdr = H.oracle_search(shards[0], q["op"], q["terms"], q["first"], q["maxitems"], q.get("window", 0), n_required=q.get("n_required", 0),
                                        reference_select_bug="coloc" in fx)
            got = [(d, w) for d, w, _ in hits[q["first"]:]]
            assert hdr.max_possible == float.fromhex(r["max_possible"])
            if "positional_edges" in fx:       # whole matches: the count is the page; the percentages: every term of a positional match matches
                assert hdr.matches == len(hits) <= H.POS_EDGE_MAX_CONJ, q
                assert not hits or hdr.max_attained == float.fromhex(r["max_attained"]), q
                pct = H.tree_percentages(hits, hdr, len(q["terms"])) if hits else []
                if "hits" not in r:            # a long page: its length and digest
                    assert (len(hits), hits_digest(hits, pct)) == (r["n_hits"], r["hits_sha256"]), q
                    continue
                assert pct == [p for _, _, p in r["hits"]], q
        else:
            got = [(d, w) for d, w, _ in H.oracle_search_sharded(shards, q["op"], q["terms"], q["first"], q["maxitems"])]
        assert got == expected(r), q
