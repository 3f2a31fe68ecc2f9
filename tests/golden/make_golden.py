"""Regenerate tests/golden/*.json from the REAL reference (oracle/_ref/xapian_ref = the vendored
Xapian of /root/reference compiled by oracle/ref_build/Makefile).  Run in the authoring container:

    python tests/golden/make_golden.py

Each fixture records the corpus parameters (tools/xgm_corpus.h), the queries, and for every query
the reference MSet: (docid, weight as a C99 hex float) per rank plus max_possible / max_attained.
Config C1 of BASELINE.json: 10k-doc synthetic index, 3-term AND BM25 top-10 through Enquire; the
other fixtures cover OR-5 top-100, full-result PHRASE, paging (first > 0), the two-sided operators
(AND_NOT / AND_MAYBE / FILTER), a 4-shard index run through Xapiand's prepare/merge protocol, and — groundwork of the
next widening row — the value sorts (sort keys recorded) and a ValueCountMatchSpy's counts over the whole match.
tree_edges.json: the nested queries of helpers.tree_edge_cases() on the crafted corpus of helpers.tree_edge_postings(), a top-10 page and the
whole match of each (`python tests/golden/make_golden.py tree_edges` writes that fixture alone).
positional_edges.json: the PHRASE / NEAR cases of helpers.positional_edge_cases() on the crafted corpus of helpers.positional_edge_postings(), the whole match
of each (`python tests/golden/make_golden.py positional_edges` writes that fixture alone).
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import helpers as H  # noqa: E402

N_DOCS, VOCAB = 10000, 1000000


def run(tmp, dbs, queries, tag, full_ranking_check=False):
    qf, of = os.path.join(tmp, tag + ".q"), os.path.join(tmp, tag + ".out")
    H.write_queries(qf, queries)
    H.xapian_ref("query", qf, of, *dbs)
    ref = H.parse_ref_output(of)
    if full_ranking_check:
        # The reference's dynamic pruning can LOSE documents for some nested shapes (an OR over AND_NOT / AND_MAYBE children,
        # DESIGN.md "reference quirks"): its top-k is then not a prefix of its own full ranking.  Such queries are recorded
        # with the prefix of the reference's FULL ranking (the intended answer, what the device returns) and flagged.
        H.write_queries(qf, [dict(q, first=0, maxitems=N_DOCS) for q in queries])
        H.xapian_ref("query", qf, of, *dbs)
        full = H.parse_ref_output(of)
        for q, r, f in zip(queries, ref, full):
            want = f["hits"][q["first"]:q["first"] + q["maxitems"]]
            if [(d, w) for d, w, _ in r["hits"]] != [(d, w) for d, w, _ in want]:
                q["reference_quirk"] = True
                r["hits"] = want
                r["max_attained"] = f["max_attained"]
    out = []
    for q, r in zip(queries, ref):
        q = {k: (list(v) if isinstance(v, tuple) else v) for k, v in q.items()}
        out.append(dict(query=q, max_possible=r["max_possible"].hex(), max_attained=r["max_attained"].hex(),
                        hits=[[d, w.hex(), pct] for d, w, pct in r["hits"]]))
        if "extra" in r:                 # sorted searches: the items' sort keys
            out[-1]["sort_keys"] = [k.hex() for k, _, _ in r["extra"]]
        if "spy" in r:                   # a ValueCountMatchSpy: documents seen, (value, count) in value order
            out[-1]["spy_total"], out[-1]["spy"] = r["spy_total"], [[v.hex(), n] for v, n in r["spy"]]
    return out


LONG_PAGE = 100


def hits_digest(hits):
    """A page too long to spell out: the SHA-256 of its lines "docid weight-as-hex-float percent"."""
    import hashlib
    return hashlib.sha256("".join("%d %s %d\n" % (d, w, p) for d, w, p in hits).encode()).hexdigest()


def tree_edges(tmp):
    """The crafted nested-query cases through the compiled reference: a top-10 page and the whole match of every case, under the same
    full-ranking rule as nested_trees (a page that is not the prefix of the reference's own whole ranking is recorded from that ranking and
    flagged — allowed only under an OR over AND_NOT / AND_MAYBE children, and for one case in eight at the most).  Whole matches of more than
    LONG_PAGE documents are recorded as their length and hits_digest."""
    post, doclen = H.tree_edge_postings()
    pf, db = os.path.join(tmp, "edges.txt"), os.path.join(tmp, "dbe")
    H.write_postings_file(pf, post, doclen)
    H.xapian_ref("build_postings", db, pf)
    cases = H.tree_edge_cases()
    results = (run(tmp, [db], H.tree_edge_queries(cases, 0, 10), "edges10", full_ranking_check=True) +
               run(tmp, [db], H.tree_edge_queries(cases, 0, H.TREE_EDGE_LASTDOCID), "edgesall", full_ranking_check=True))
    flagged = sorted({r["query"]["name"] for r in results if r["query"].get("reference_quirk")})
    assert all(H.tree_has_or_over_sided(dict(cases)[n]) for n in flagged), flagged
    assert len(flagged) * 8 <= len(cases), flagged
    for r in results:
        if len(r["hits"]) > LONG_PAGE:
            r["n_hits"], r["hits_sha256"] = len(r["hits"]), hits_digest(r["hits"])
            del r["hits"]
    with open(os.path.join(HERE, "tree_edges.json"), "w") as f:
        json.dump(dict(tree_edges=dict(lastdocid=H.TREE_EDGE_LASTDOCID), n_shards=1, results=results), f, indent=0)
    print("tree_edges: %d cases, flagged as reference quirks: %s" % (len(cases), flagged))


def positional_edges(tmp):
    """The crafted positional cases through the compiled reference: the whole match of every case (maxitems covers the conjunction, so neither the
    stale SelectPostList weight nor NEAR's history can engage: positions inside a document are distinct).  A case the reference itself crashes on
    would be recorded without an answer and named; at most three may."""
    import subprocess
    post, doclen = H.positional_edge_postings()
    pf, db = os.path.join(tmp, "pos.txt"), os.path.join(tmp, "dbp")
    H.write_postings_file(pf, post, doclen)
    H.xapian_ref("build_postings", db, pf)
    cases = H.positional_edge_cases()
    try:
        results, crashed = run(tmp, [db], cases, "posedges"), []
    except subprocess.CalledProcessError:                          # one by one: which case takes the reference down
        results, crashed = [], []
        for c in cases:
            try:
                results += run(tmp, [db], [c], "posedge1")
            except subprocess.CalledProcessError:
                crashed.append(c["name"])
                results.append(dict(query=c, reference_crashed=True))
    assert len(crashed) <= 3, crashed
    for r in results:
        if len(r.get("hits", ())) > LONG_PAGE:
            r["n_hits"], r["hits_sha256"] = len(r["hits"]), hits_digest(r["hits"])
            del r["hits"]
    with open(os.path.join(HERE, "positional_edges.json"), "w") as f:
        json.dump(dict(positional_edges=dict(lastdocid=H.POS_EDGE_LASTDOCID, seed=H.POS_EDGE_SEED), n_shards=1, results=results), f, indent=0)
    print("positional_edges: %d cases, the reference crashed on: %s" % (len(cases), crashed))


def sharded(tmp, corpus, n_shards):
    """Xapiand's per-shard protocol (prepare_mset / add_prepared_mset / get_mset per shard / unshard_docids + merge_mset, handler.cc:1532-1549)
    over n_shards docid-interleaved shards (multi.h:38-73) through the compiled reference: 4 shards (rounds 1-4) and — C4's shape, the
    8-GPU node — 8 (round 5)."""
    dbs = []
    for s in range(n_shards):
        d = os.path.join(tmp, "s%d_%d" % (n_shards, s))
        H.xapian_ref("build", d, H.CORPUS_SEED, N_DOCS, VOCAB, 50, 150, n_shards, s)
        dbs.append(d)
    qs = H.gen_term_queries("AND", 30, 3, 1, 64, maxitems=10, seed=24) + H.gen_term_queries("OR", 10, 5, 8, 4096, maxitems=20, seed=25)
    with open(os.path.join(HERE, "sharded%d_and3_top10.json" % n_shards), "w") as f:
        json.dump(dict(corpus=corpus, n_shards=n_shards, results=run(tmp, dbs, qs, "sh%d" % n_shards)), f, indent=0)


def main():
    if sys.argv[1:] == ["sharded8"]:              # only the 8-shard fixture (the others are unchanged: same generator, same reference)
        with tempfile.TemporaryDirectory() as tmp:
            sharded(tmp, dict(seed=H.CORPUS_SEED, n_docs=N_DOCS, vocab=VOCAB, len_lo=50, len_hi=150), 8)
        print("sharded8 fixture written to", HERE)
        return
    if sys.argv[1:] == ["tree_edges"]:
        with tempfile.TemporaryDirectory() as tmp:
            tree_edges(tmp)
        return
    if sys.argv[1:] == ["positional_edges"]:
        with tempfile.TemporaryDirectory() as tmp:
            positional_edges(tmp)
        return
    with tempfile.TemporaryDirectory() as tmp:
        db = os.path.join(tmp, "db")
        H.xapian_ref("build", db, H.CORPUS_SEED, N_DOCS, VOCAB, 50, 150)
        corpus = dict(seed=H.CORPUS_SEED, n_docs=N_DOCS, vocab=VOCAB, len_lo=50, len_hi=150)
        fixtures = {
            "c1_and3_top10": H.gen_term_queries("AND", 60, 3, 1, 64, maxitems=10),
            "or5_top100": H.gen_term_queries("OR", 30, 5, 8, 4096, maxitems=100, seed=21),
            "and_paging": H.gen_term_queries("AND", 10, 2, 1, 64, first=7, maxitems=10, seed=22),
            "phrase_full": H.gen_phrase_queries(30, N_DOCS, VOCAB, maxitems=N_DOCS, seed=23),
            # the operators of Xapiand's _and_not / _and_maybe / _filter (left = AND of n_required terms)
            "sided_top10": sum((H.gen_sided_queries(op, 12, 1, 1, 1, 300, maxitems=10, seed=sd) +
                                H.gen_sided_queries(op, 12, 2, 2, 1, 64, 1, 600, maxitems=10, seed=sd + 1) +
                                H.gen_sided_queries(op, 6, 3, 1, 1, 40, 1, 40, first=4, maxitems=10, seed=sd + 2)
                                for op, sd in (("AND_NOT", 31), ("AND_MAYBE", 41), ("FILTER", 51))), []),
        }
        # nested operator trees / OP_SYNONYM / OP_SCALE_WEIGHT / wqf, in xapian_ref's post-order "RPN" form
        tq = H.gen_tree_queries(72, 1, 300, seed=61)
        for q in tq[36:]:
            q["maxitems"] = 40
        fixtures["nested_trees"] = tq
        for name, qs in fixtures.items():
            with open(os.path.join(HERE, name + ".json"), "w") as f:
                json.dump(dict(corpus=corpus, n_shards=1, results=run(tmp, [db], qs, name, full_ranking_check=name == "nested_trees")), f, indent=0)
        # widening row (f).3: value sorts and a ValueCountMatchSpy on the corpus's three value slots (tools/xgm_corpus.h)
        import random
        dbv = os.path.join(tmp, "dbv")
        H.xapian_ref("build_values", dbv, H.CORPUS_SEED, N_DOCS, VOCAB, 50, 150)
        rng = random.Random(71)
        base = (H.gen_term_queries("OR", 10, 3, 1, 300, maxitems=10, seed=72) + H.gen_term_queries("AND", 10, 2, 1, 40, maxitems=10, seed=73) +
                H.gen_sided_queries("AND_MAYBE", 5, 1, 2, 1, 200, maxitems=10, seed=74) + H.gen_term_queries("OR", 5, 2, 1, 2000, first=7, maxitems=9, seed=75))
        sorted_qs = [dict(q, sort=[rng.choice(["V", "VR", "RV"]), rng.randrange(3), rng.random() < 0.5]) for q in base for _ in range(2)]
        # (slots 0 and 2, the categories: slot 1 has nearly a distinct value per document — that one is pinned live, tests/test_oracle_vs_reference.py)
        spy_qs = [dict(q, spy=rng.choice([0, 2]), check_at_least=N_DOCS) for q in base]
        for name, qs in (("sorted_values", sorted_qs), ("spy_counts", spy_qs)):
            with open(os.path.join(HERE, name + ".json"), "w") as f:
                json.dump(dict(corpus=corpus, n_shards=1, results=run(tmp, [dbv], qs, name)), f, indent=0)
        # NEAR over co-located terms (nearpostlist.cc:106-140): hand-made documents with several terms per position (helpers.coloc_postings),
        # built posting by posting; the reference's answers INCLUDE its history dependence: the oracle's reference mode
        # must reproduce them query by query, top-10 pages too
        post, doclen = H.coloc_postings()
        pf, dbc = os.path.join(tmp, "coloc.txt"), os.path.join(tmp, "dbc")
        H.write_postings_file(pf, post, doclen)
        H.xapian_ref("build_postings", dbc, pf)
        with open(os.path.join(HERE, "near_colocated.json"), "w") as f:
            json.dump(dict(coloc=dict(seed=0xC010C, n_docs=600), n_shards=1, results=run(tmp, [dbc], H.coloc_near_queries(), "coloc")), f, indent=0)
        tree_edges(tmp)
        positional_edges(tmp)
        sharded(tmp, corpus, 4)
        sharded(tmp, corpus, 8)
    print("golden fixtures written to", HERE)


if __name__ == "__main__":
    main()
