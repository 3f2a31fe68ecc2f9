"""Test-side helpers: ctypes binding of the CPU oracle (oracle/libxgm_oracle.so), the runner of the
real-reference binary (oracle/_ref/xapian_ref), seeded query generators and the glue that feeds the
oracle's raw postings to the product's segment builder.  Only tests/, smoke() and bench.py's
cpu_baseline leg import this module."""
import ctypes as C
import os
import random
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_LIB = os.path.join(ROOT, "oracle", "libxgm_oracle.so")
XAPIAN_REF = os.path.join(ROOT, "oracle", "_ref", "xapian_ref")

CORPUS_SEED = 0x5EED0001
QUERY_SEED = 0x5EED0002
OPS = {"AND": 1, "OR": 2, "PHRASE": 3, "AND_NOT": 4, "AND_MAYBE": 5, "FILTER": 6, "NEAR": 7}   # NEAR: oracle only so far
SIDED = ("AND_NOT", "AND_MAYBE", "FILTER")   # left = AND of the first n_required terms, right = the others


MATCHES_LOWER_BOUND = 1 << 63      # include/xgm.h: XGM_MATCHES_LOWER_BOUND
EXACT_COUNT = 0x7FFFFFFF           # a check_at_least that asks for the exact match count of a positional query


def check_matches(got_raw, want, n_hits, what=None):
    """xgm_result_hdr.matches_exact against the oracle's count: exact — or, flagged (a positional query answered with
    check_at_least inside the page: candidates that cannot rank are dropped before their positions are tested), a lower
    bound that still covers the hits returned."""
    if got_raw & MATCHES_LOWER_BOUND:
        cnt = got_raw & ~MATCHES_LOWER_BOUND
        assert n_hits <= cnt <= want, (what, cnt, want, n_hits)
    else:
        assert got_raw == want, (what, got_raw, want)


class CorpusView(C.Structure):
    _fields_ = [("n_terms", C.c_uint32), ("lastdocid", C.c_uint32), ("doccount", C.c_uint32),
                ("has_positions", C.c_uint32), ("total_length", C.c_uint64), ("n_postings", C.c_uint64),
                ("n_positions", C.c_uint64),
                ("doclen", C.POINTER(C.c_uint32)), ("terms", C.POINTER(C.c_char_p)),
                ("term_len", C.POINTER(C.c_uint32)), ("df", C.POINTER(C.c_uint32)),
                ("did", C.POINTER(C.c_uint32)), ("wdf", C.POINTER(C.c_uint32)),
                ("pos_off", C.POINTER(C.c_uint64)), ("pos", C.POINTER(C.c_uint32))]


class OHit(C.Structure):
    _fields_ = [("docid", C.c_uint32), ("subqs", C.c_uint32), ("weight", C.c_double)]


class OHdr(C.Structure):
    _fields_ = [("n_hits", C.c_uint32), ("max_subqs", C.c_uint32), ("matches", C.c_uint64),
                ("max_attained", C.c_double), ("max_possible", C.c_double)]


_olib = None


def olib():
    global _olib
    if _olib is None:
        l = C.CDLL(ORACLE_LIB)
        l.xgo_corpus_build.restype = C.c_void_p
        l.xgo_corpus_build.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
        l.xgo_corpus_build_terms.restype = C.c_void_p
        l.xgo_corpus_build_terms.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_uint32),
                                             C.c_uint32, C.c_uint32]
        l.xgo_corpus_free.argtypes = [C.c_void_p]
        l.xgo_corpus_get.argtypes = [C.c_void_p, C.POINTER(CorpusView)]
        l.xgo_index_from_raw.restype = C.c_void_p
        l.xgo_index_from_raw.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32),
                                         C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                         C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint32)]
        l.xgo_index_free.argtypes = [C.c_void_p]
        l.xgo_index_termfreq.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32]
        l.xgo_index_warm.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32]
        l.xgo_search.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), C.c_uint32,
                                 C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32,
                                 C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(OHit), C.POINTER(OHdr)]
        _olib = l
    return _olib


class Corpus:
    """Deterministic synthetic corpus shard (tools/xgm_corpus.h) inverted to raw postings by the oracle."""

    def __init__(self, n_docs_global, vocab, seed=CORPUS_SEED, len_lo=50, len_hi=150, n_shards=1, shard=0, positions=True):
        self.params = dict(seed=seed, n_docs_global=n_docs_global, vocab=vocab, len_lo=len_lo, len_hi=len_hi,
                           n_shards=n_shards, shard=shard)
        self._h = olib().xgo_corpus_build(seed, n_docs_global, vocab, len_lo, len_hi, n_shards, shard, 1 if positions else 0)
        self.v = CorpusView()
        olib().xgo_corpus_get(self._h, C.byref(self.v))
        self._oidx = None

    def close(self):
        if self._oidx:
            olib().xgo_index_free(self._oidx)
            self._oidx = None
        if self._h:
            olib().xgo_corpus_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def terms(self):
        return [C.string_at(self.v.terms[i], self.v.term_len[i]) for i in range(self.v.n_terms)]

    def df_array(self):
        return np.ctypeslib.as_array(self.v.df, shape=(self.v.n_terms,))

    def term_postings(self, idx):
        df = self.df_array()
        start = int(df[:idx].sum())
        n = int(df[idx])
        did = np.ctypeslib.as_array(self.v.did, shape=(self.v.n_postings,))[start:start + n]
        wdf = np.ctypeslib.as_array(self.v.wdf, shape=(self.v.n_postings,))[start:start + n]
        return did, wdf

    def raw_postings(self, revision=1):
        """Fill the product's xgm_raw_postings from the oracle's arrays (borrowed pointers)."""
        from xapiand_amd import _lib
        r = _lib.RawPostings()
        v = self.v
        r.n_terms, r.lastdocid, r.doccount, r.has_positions = v.n_terms, v.lastdocid, v.doccount, v.has_positions
        r.total_length, r.n_postings, r.n_positions, r.revision = v.total_length, v.n_postings, v.n_positions, revision
        r.doclen, r.terms, r.term_len, r.df, r.did, r.wdf = v.doclen, v.terms, v.term_len, v.df, v.did, v.wdf
        r.pos_off, r.pos = v.pos_off, v.pos
        return r

    def build_segment(self, path, stripe_bits=0, revision=1):
        from xapiand_amd import _lib
        r = self.raw_postings(revision)
        _lib.check(_lib.lib().xgm_segment_build(C.byref(r), stripe_bits, path.encode()))
        return path

    def oracle_index(self):
        if self._oidx is None:
            v = self.v
            self._oidx = olib().xgo_index_from_raw(v.n_terms, v.lastdocid, v.doccount, v.total_length, v.doclen, v.terms,
                                                   v.term_len, v.df, v.did, v.wdf, v.pos_off, v.pos)
        return self._oidx

    def termfreq(self, term):
        t = term if isinstance(term, bytes) else term.encode()
        return olib().xgo_index_termfreq(self.oracle_index(), t, len(t))


def oracle_search(corpus, op, terms, first, maxitems, window=0, global_stats=None, reference_select_bug=False, n_required=0):
    """Run the CPU oracle.  Returns (list of (docid, weight, subqs), hdr)."""
    n = len(terms)
    opcode = OPS[op] | ((n_required or 1) << 8 if op in SIDED else 0)
    tb = [t if isinstance(t, bytes) else t.encode() for t in terms]
    arr = (C.c_char_p * n)(*tb)
    lens = (C.c_uint32 * n)(*[len(t) for t in tb])
    cap = max(1, first + maxitems)
    hits = (OHit * cap)()
    hdr = OHdr()
    bug = 1 if reference_select_bug else 0
    if global_stats is None:
        rc = olib().xgo_search(corpus.oracle_index(), opcode, n, arr, lens, window, first, maxitems, 0, 0, 0, 0, None, bug, hits, C.byref(hdr))
    else:
        tf = (C.c_uint32 * n)(*global_stats["termfreq"])
        rc = olib().xgo_search(corpus.oracle_index(), opcode, n, arr, lens, window, first, maxitems, 1,
                               global_stats["total_length"], global_stats["collection_size"],
                               1 if global_stats["has_positions"] else 0, tf, bug, hits, C.byref(hdr))
    assert rc == 0
    return [(hits[i].docid, hits[i].weight, hits[i].subqs) for i in range(hdr.n_hits)], hdr


SORT_MODES = {"V": 1, "VR": 2, "RV": 3}      # Enquire::set_sort_by_value / _value_then_relevance / _relevance_then_value


def oracle_search_sorted(corpus, op, terms, first, maxitems, mode, slot, reverse, n_required=0, collapse=None, global_stats=None):
    """The oracle with a value sort (mode "V" / "VR" / "RV"; None = relevance) and / or a collapse (slot, collapse_max) in force
    (widening row (f).3; corpus value slots: tools/xgm_corpus.h).  Returns (list of (docid, weight, subqs, sort_key bytes),
    hdr) — with collapse: (docid, weight, subqs, sort_key, collapse_key, collapse_count) and hdr.collapsed_lower_bound."""
    ol = olib()
    ol.xgo_index_set_synthetic_values.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32]
    ol.xgo_search_sorted_g.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32,
                                       C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(OHit), C.POINTER(OHdr), C.c_char_p, C.c_uint32,
                                       C.c_uint32, C.c_uint32, C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                       C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    if not getattr(corpus, "_values_set", False):
        ol.xgo_index_set_synthetic_values(corpus.oracle_index(), corpus.params["seed"], corpus.params["n_shards"], corpus.params["shard"])
        corpus._values_set = True
    n = len(terms)
    opcode = OPS[op] | ((n_required or 1) << 8 if op in SIDED else 0)
    tb = [t if isinstance(t, bytes) else t.encode() for t in terms]
    arr = (C.c_char_p * n)(*tb)
    lens = (C.c_uint32 * n)(*[len(t) for t in tb])
    cap = max(1, first + maxitems)
    hits = (OHit * cap)()
    hdr = OHdr()
    keys, ckeys = C.create_string_buffer(cap * 8), C.create_string_buffer(cap * 8)
    ccounts = (C.c_uint32 * cap)()
    clb = C.c_uint64()
    cslot, cmax = collapse if collapse else (0, 0)
    gs = global_stats
    tf = (C.c_uint32 * n)(*gs["termfreq"]) if gs else None
    rc = ol.xgo_search_sorted_g(corpus.oracle_index(), opcode, n, arr, lens, 0, first, maxitems, SORT_MODES[mode] if mode else 0, slot, 1 if reverse else 0,
                                hits, C.byref(hdr), keys, 8, cslot, cmax, ckeys, ccounts, C.byref(clb),
                                1 if gs else 0, gs["total_length"] if gs else 0, gs["collection_size"] if gs else 0,
                                (1 if gs["has_positions"] else 0) if gs else 0, tf)
    assert rc == 0
    raw, craw = keys.raw, ckeys.raw
    hdr.collapsed_lower_bound = clb.value
    if collapse:
        return [(hits[i].docid, hits[i].weight, hits[i].subqs, raw[8 * i:8 * i + 8].rstrip(b"\0"), craw[8 * i:8 * i + 8].rstrip(b"\0"), ccounts[i]) for i in range(hdr.n_hits)], hdr
    return [(hits[i].docid, hits[i].weight, hits[i].subqs, raw[8 * i:8 * i + 8].rstrip(b"\0")) for i in range(hdr.n_hits)], hdr


def oracle_search_sharded(corpora, op, terms, first, maxitems, window=0):
    """Xapiand's per-shard protocol on the oracle: merged stats, per-shard top first+maxitems, unshard, merge."""
    gs = dict(total_length=sum(c.v.total_length for c in corpora), collection_size=sum(c.v.doccount for c in corpora),
              has_positions=any(c.v.has_positions for c in corpora),
              termfreq=[sum(c.termfreq(t) for c in corpora) for t in terms])
    n = len(corpora)
    allhits = []
    for s, c in enumerate(corpora):
        hits, _ = oracle_search(c, op, terms, 0, first + maxitems, window, gs)
        allhits += [((d - 1) * n + s + 1, w, m) for d, w, m in hits]
    allhits.sort(key=lambda x: (-x[1], x[0]))
    return allhits[first:first + maxitems]


def oracle_spy(corpus, op, terms, slot, window=0, n_required=0):
    """A ValueCountMatchSpy on `slot` over every document the query matches (corpus value slots: tools/xgm_corpus.h).
    Returns (documents seen, [(value, count)] in value order)."""
    ol = olib()
    ol.xgo_index_set_synthetic_values.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32]
    ol.xgo_search_spy.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32,
                                  C.c_uint32, C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    if not getattr(corpus, "_values_set", False):
        ol.xgo_index_set_synthetic_values(corpus.oracle_index(), corpus.params["seed"], corpus.params["n_shards"], corpus.params["shard"])
        corpus._values_set = True
    n = len(terms)
    opcode = OPS[op] | ((n_required or 1) << 8 if op in SIDED else 0)
    tb = [t if isinstance(t, bytes) else t.encode() for t in terms]
    arr = (C.c_char_p * n)(*tb)
    lens = (C.c_uint32 * n)(*[len(t) for t in tb])
    cap = 1 << 20
    values, counts = C.create_string_buffer(cap * 8), (C.c_uint32 * cap)()
    nv, total = C.c_uint32(), C.c_uint64()
    assert ol.xgo_search_spy(corpus.oracle_index(), opcode, n, arr, lens, window, slot, cap, 8, values, counts, C.byref(nv), C.byref(total)) == 0
    raw = values.raw
    return total.value, [(raw[8 * i:8 * i + 8].rstrip(b"\0"), counts[i]) for i in range(nv.value)]


def oracle_search_sharded_sorted(corpora, op, terms, first, maxitems, mode, slot, reverse):
    """oracle_search_sharded under a value sort: every shard's first + maxitems best under the comparison, merged under the same
    comparison over global docids (matcher/msetcmp.cc:64-101).  Returns [(global docid, weight, subqs, sort key)]."""
    import functools
    gs = dict(total_length=sum(c.v.total_length for c in corpora), collection_size=sum(c.v.doccount for c in corpora),
              has_positions=any(c.v.has_positions for c in corpora),
              termfreq=[sum(c.termfreq(t) for c in corpora) for t in terms])
    n = len(corpora)
    allhits = []
    for s, c in enumerate(corpora):
        hits, _ = oracle_search_sorted(c, op, terms, 0, first + maxitems, mode, slot, reverse, global_stats=gs)
        allhits += [((d - 1) * n + s + 1, w, m, k) for d, w, m, k in hits]

    def cmp(a, b):
        if mode == "RV" and a[1] != b[1]:
            return -1 if a[1] > b[1] else 1
        if a[3] != b[3]:
            return (-1 if a[3] > b[3] else 1) if reverse else (-1 if a[3] < b[3] else 1)
        if mode == "VR" and a[1] != b[1]:
            return -1 if a[1] > b[1] else 1
        return -1 if a[0] < b[0] else (1 if a[0] > b[0] else 0)
    allhits.sort(key=functools.cmp_to_key(cmp))
    return allhits[first:first + maxitems]


# ---- the real reference -------------------------------------------------------------------------

def have_xapian_ref():
    return os.path.exists(XAPIAN_REF)


def xapian_ref(*args):
    return subprocess.run([XAPIAN_REF] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout


def write_queries(path, queries):
    with open(path, "w") as f:
        for q in queries:
            op = q["op"] + (":%d" % (q.get("n_required") or 1) if q["op"] in SIDED else "")
            pre = ""
            if q.get("sort"):
                pre += "SORT=%s:%d:%d " % (q["sort"][0], q["sort"][1], 1 if q["sort"][2] else 0)
            if q.get("collapse"):
                pre += "COLLAPSE=%d:%d " % tuple(q["collapse"])
            if q.get("check_at_least"):
                pre += "CAL=%d " % q["check_at_least"]
            if q.get("spy") is not None:
                if q.get("spy_aggregation"):
                    pre += "SPYA=%d:%d " % (q["spy"], q.get("agg_kind", 0))          # Xapiand's own AggregationMatchSpy; kind: oracle/ref_build/xapiand_classes.cc aggs_conf
                else:
                    pre += ("SPYC=%d " if q.get("spy_custom") else "SPY=%d ") % q["spy"]
            if q.get("cutoff"):
                pre += "CUT=%d:%r " % (q["cutoff"][0], float(q["cutoff"][1]))
            f.write("%s%s %d %d %d %s\n" % (pre, op, q["first"], q["maxitems"], q.get("window", 0), " ".join(q["terms"])))


def parse_ref_output(path):
    """Parse xapian_ref query output → list of dicts with exact (hex) weights."""
    out = []
    with open(path) as f:
        for line in f:
            p = line.split()
            if p[0] == "Q":
                out.append(dict(n=int(p[2]), lb=int(p[3]), est=int(p[4]), ub=int(p[5]), max_possible=float.fromhex(p[6]),
                                max_attained=float.fromhex(p[7]), hits=[]))
            elif p[0] == "H":
                out[-1]["hits"].append((int(p[2]), float.fromhex(p[3]), int(p[4])))
            elif p[0] == "X":       # sorted / collapsed searches: sort key, collapse key (hex, "-" = empty), collapse count
                out[-1].setdefault("extra", []).append((b"" if p[2] == "-" else bytes.fromhex(p[2]), b"" if p[3] == "-" else bytes.fromhex(p[3]), int(p[4])))
            elif p[0] == "U":
                out[-1]["uncollapsed"] = (int(p[1]), int(p[2]), int(p[3]))
            elif p[0] == "S":       # a ValueCountMatchSpy: documents it saw, then one V line per distinct value
                out[-1]["spy_total"], out[-1]["spy"] = int(p[1]), []
            elif p[0] == "V":
                out[-1]["spy"].append((bytes.fromhex(p[1]), int(p[2])))
    return out


# ---- seeded query generators ---------------------------------------------------

def log_uniform_rank(rng, lo, hi):
    import math
    return int(round(math.exp(rng.uniform(math.log(lo), math.log(hi)))))


def gen_term_queries(op, n_queries, n_terms, rank_lo, rank_hi, first=0, maxitems=10, seed=QUERY_SEED):
    rng = random.Random(seed)
    qs = []
    for _ in range(n_queries):
        ranks = set()
        while len(ranks) < n_terms:
            ranks.add(max(1, log_uniform_rank(rng, rank_lo, rank_hi)))
        ranks = list(ranks)
        rng.shuffle(ranks)
        qs.append(dict(op=op, terms=["t%d" % r for r in ranks], first=first, maxitems=maxitems, window=0))
    return qs


def gen_sided_queries(op, n_queries, n_required, n_other, rank_lo, rank_hi, other_lo=None, other_hi=None, first=0, maxitems=10, seed=QUERY_SEED):
    """AND_NOT / AND_MAYBE / FILTER: the first n_required terms form the left-hand AND, n_other terms the
    right-hand side (ranks from their own range when given)."""
    rng = random.Random(seed)
    qs = []
    for _ in range(n_queries):
        ranks = []
        while len(ranks) < n_required:
            r = max(1, log_uniform_rank(rng, rank_lo, rank_hi))
            if r not in ranks:
                ranks.append(r)
        while len(ranks) < n_required + n_other:
            r = max(1, log_uniform_rank(rng, other_lo or rank_lo, other_hi or rank_hi))
            if r not in ranks:
                ranks.append(r)
        qs.append(dict(op=op, n_required=n_required, terms=["t%d" % r for r in ranks], first=first, maxitems=maxitems, window=0))
    return qs


def hash64(seed, a, b):
    """tools/xgm_corpus.h xgm_hash3 in Python ints."""
    M = (1 << 64) - 1

    def mix(z):
        z = (z + 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    return mix(mix(seed ^ ((a * 0xD6E8FEB86659FD93) & M)) ^ ((b * 0xA0761D6478BD642F) & M))


_thr_cache = {}


def zipf_thresholds(vocab):
    if vocab not in _thr_cache:
        inv = 1.0 / np.arange(1, vocab + 1, dtype=np.float64)
        # sequential summation exactly like the C code (np.cumsum is sequential for float64)
        h = np.cumsum(inv)
        hv = 0.0
        for x in inv:       # same order of additions as xgm_zipf_thresholds' first loop
            hv += x
        f = h / hv
        hi = f * 4294967296.0
        hi_i = np.floor(hi)
        lo = (hi - hi_i) * 4294967296.0
        thr = (hi_i.astype(np.uint64) << np.uint64(32)) | np.floor(lo).astype(np.uint64)
        thr[-1] = np.uint64(0xFFFFFFFFFFFFFFFF)
        thr[f >= 1.0] = np.uint64(0xFFFFFFFFFFFFFFFF)
        _thr_cache[vocab] = thr
    return _thr_cache[vocab]


def doc_tokens(seed, vocab, len_lo, len_hi, g):
    """Tokens (ranks) of global doc g — Python restatement of the corpus for phrase-query sampling."""
    thr = zipf_thresholds(vocab)
    n = len_lo + hash64(seed, g, 0xFFFFFFFF) % (len_hi - len_lo + 1)
    toks = []
    for pos in range(1, n + 1):
        u = np.uint64(hash64(seed, g, pos))
        toks.append(int(np.searchsorted(thr, u, side="right")) + 1 if u >= thr[0] else 1)
    return toks


def gen_phrase_queries(n_queries, n_docs_global, vocab, len_lo=50, len_hi=150, corpus_seed=CORPUS_SEED, seed=QUERY_SEED,
                       maxitems=10, window_extra=0, lengths=(2, 3), op="PHRASE"):
    """2-3-grams that actually occur in a random document (so results are non-empty); n-grams with a
    repeated term are skipped (the device path declines them, like any other unsupported shape)."""
    rng = random.Random(seed)
    qs = []
    while len(qs) < n_queries:
        g = rng.randint(1, n_docs_global)
        toks = doc_tokens(corpus_seed, vocab, len_lo, len_hi, g)
        n = rng.choice(list(lengths))
        i = rng.randint(0, len(toks) - n)
        gram = toks[i:i + n]
        if len(set(gram)) != n:
            continue
        qs.append(dict(op=op, terms=["t%d" % r for r in gram], first=0, maxitems=maxitems,
                       window=(n + window_extra) if window_extra else 0))
    return qs


def bench_pool(op, n_terms=3, n_required=1, n_docs_global=10_000_000, vocab=1_000_000, n=1100, seed=QUERY_SEED, maxitems=10):
    """The query pool of bench.py (ranks log-uniform in [8, 4096], no repetition inside a query; PHRASE:
    2-3-grams that occur in a random document) as query dicts.  bench.py warms up on the first 100 and times the
    rest; the config-scale parity tests check the first queries of the timed part."""
    import math
    if op == "PHRASE":
        return gen_phrase_queries(n, n_docs_global, vocab, seed=seed, maxitems=maxitems)
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        ranks = set()
        while len(ranks) < n_terms:
            ranks.add(max(1, int(round(math.exp(rng.uniform(math.log(8), math.log(4096)))))))
        ranks = list(ranks)
        rng.shuffle(ranks)
        out.append(dict(op=op, terms=["t%d" % r for r in ranks], first=0, maxitems=maxitems, window=0,
                        n_required=n_required if op in SIDED else 0))
    return out


class TermsCorpus(Corpus):
    """The synthetic corpus inverted on the HOST (oracle/xgm_oracle.cc::corpus_build_terms, tools/xgm_corpus.h) for a handful of terms only: every document is
    generated — lengths and statistics are the whole shard's —, only the postings of `terms` ("t<rank>") are kept.  What feeds the oracle at a
    configuration's full size WITHOUT reading anything back from the device (DeviceOracle does); same interface as Corpus for the oracle functions."""

    def __init__(self, n_docs_global, vocab, terms, seed=CORPUS_SEED, len_lo=50, len_hi=150, n_shards=1, shard=0, positions=False, n_threads=None):
        ranks = sorted({int((t.decode() if isinstance(t, bytes) else t)[1:]) for t in terms})
        arr = (C.c_uint32 * len(ranks))(*ranks)
        self.params = dict(seed=seed, n_docs_global=n_docs_global, vocab=vocab, len_lo=len_lo, len_hi=len_hi, n_shards=n_shards, shard=shard)
        self._h = olib().xgo_corpus_build_terms(seed, n_docs_global, vocab, len_lo, len_hi, n_shards, shard, 1 if positions else 0, arr, len(ranks),
                                                n_threads or max(1, os.cpu_count() or 1))
        self.v = CorpusView()
        olib().xgo_corpus_get(self._h, C.byref(self.v))
        self._oidx = None

    def warm(self):
        for i in range(self.v.n_terms):
            olib().xgo_index_warm(self.oracle_index(), self.v.terms[i], self.v.term_len[i])


class ManualCorpus(Corpus):
    """Hand-made postings: {term: [(docid, wdf, [positions...]), ...]} plus doc lengths.  Same
    interface as Corpus so it can feed both the oracle and the segment builder."""

    def __init__(self, postings, doclen, positions=True):
        terms = sorted((t if isinstance(t, bytes) else t.encode()) for t in postings)
        by = {(t if isinstance(t, bytes) else t.encode()): v for t, v in postings.items()}
        lastdocid = max(doclen) if doclen else 0
        self._doclen = np.zeros(lastdocid + 1, dtype=np.uint32)
        for d, l in doclen.items():
            self._doclen[d] = l
        df, did, wdf, pos_off, pos = [], [], [], [0], []
        for t in terms:
            plist = sorted(by[t])
            df.append(len(plist))
            for p in plist:
                did.append(p[0]); wdf.append(p[1])
                pp = list(p[2]) if len(p) > 2 and p[2] is not None else []
                pos += pp
                pos_off.append(len(pos))
        self._df = np.array(df, dtype=np.uint32)
        self._did = np.array(did, dtype=np.uint32)
        self._wdf = np.array(wdf, dtype=np.uint32)
        self._pos_off = np.array(pos_off, dtype=np.uint64)
        self._pos = np.array(pos if pos else [0], dtype=np.uint32)
        self._term_len = np.array([len(t) for t in terms], dtype=np.uint32)
        self._terms = (C.c_char_p * len(terms))(*terms)
        self._term_bytes = terms
        v = CorpusView()
        v.n_terms, v.lastdocid = len(terms), lastdocid
        v.doccount = int((self._doclen > 0).sum())
        v.has_positions = 1 if positions else 0
        v.total_length = int(self._doclen.sum())
        v.n_postings, v.n_positions = len(did), len(pos)
        u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
        v.doclen = self._doclen.ctypes.data_as(u32p)
        v.terms = C.cast(self._terms, C.POINTER(C.c_char_p))
        v.term_len = self._term_len.ctypes.data_as(u32p)
        v.df = self._df.ctypes.data_as(u32p)
        v.did = self._did.ctypes.data_as(u32p)
        v.wdf = self._wdf.ctypes.data_as(u32p)
        if positions:
            v.pos_off = self._pos_off.ctypes.data_as(u64p)
            v.pos = self._pos.ctypes.data_as(u32p)
        self.v = v
        self._h = None
        self._oidx = None
        self.params = None

    def terms(self):
        return list(self._term_bytes)

    def set_values(self, slot, values):
        """One value slot of the oracle's index from {docid: bytes} (at most 7 bytes each: the oracle hands keys out with a stride of 8; a docid
        left out, or b"", has no value).  After it oracle_search_sorted / oracle_spy work on this corpus, and write_value_column writes the slot."""
        last = self.v.lastdocid
        assert all(1 <= d <= last and len(v) <= 7 for d, v in values.items())
        off = np.zeros(last + 2, dtype=np.uint64)
        off[1:] = np.cumsum([len(values.get(d, b"")) for d in range(last + 1)], dtype=np.uint64)
        blob = b"".join(values.get(d, b"") for d in range(last + 1))
        ol = olib()
        ol.xgo_index_set_values.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.c_char_p]
        assert ol.xgo_index_set_values(self.oracle_index(), slot, off.ctypes.data_as(C.POINTER(C.c_uint64)), blob) == 0
        self._values_set = True


def write_value_column(corpus, slot, path):
    """The oracle's value slot as a column file (oracle/xgm_oracle.cc::xgo_write_value_column); the slots must be set."""
    assert getattr(corpus, "_values_set", False)
    ol = olib()
    ol.xgo_write_value_column.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p]
    assert ol.xgo_write_value_column(corpus.oracle_index(), slot, path.encode()) == 0
    return path


def coloc_postings(seed=0xC010C, n_docs=600):
    """Documents whose indexer puts SEVERAL TERMS AT ONE POSITION (a word's prefixed and unprefixed forms, synonyms): what engages the
    duplicate-position step of NearPostList::test_doc (nearpostlist.cc:106-140).  Returns (postings {term: [(did, wdf, [pos...])]}, doclen
    {did: length}) for ManualCorpus; write_postings_file() spells the same documents out for `xapian_ref build_postings`.  Five query terms
    ca..ce — ca / cb mostly TOGETHER on a position, cc often with one of them, cd / ce on positions of their own — among fillers."""
    import random
    rng = random.Random(seed)
    post, doclen = {}, {}
    for d in range(1, n_docs + 1):
        at = {}                                      # position -> set of terms
        n_pos = rng.randrange(12, 40)
        for p in range(1, n_pos + 1):
            r = rng.random()
            here = set()
            if r < 0.10: here |= {"ca", "cb"}
            elif r < 0.16: here.add("ca")
            elif r < 0.22: here.add("cb")
            if rng.random() < 0.12: here.add("cc")
            if rng.random() < 0.07: here.add(rng.choice(["cd", "ce"]))
            if rng.random() < 0.03: here |= {"cd", "ce"}
            if not here or rng.random() < 0.5: here.add("f%d" % rng.randrange(30))
            at[p] = here
        by = {}
        for p in sorted(at):
            for t in at[p]:
                by.setdefault(t, []).append(p)
        for t, pp in by.items():
            post.setdefault(t, []).append((d, len(pp), pp))
        doclen[d] = sum(len(pp) for pp in by.values())
    return post, doclen


def write_postings_file(path, post, doclen):
    docs = {}
    for t, pl in post.items():
        for d, _, pp in pl:
            docs.setdefault(d, []).extend("%s:%d" % (t, p) for p in pp)
    with open(path, "w") as f:
        for d in range(1, max(doclen) + 1):
            f.write((" ".join(sorted(docs.get(d, []))) if d in doclen else "-") + "\n")      # "-": a deleted document, its docid a gap


def coloc_near_queries():
    qs = []
    for terms in (["ca", "cb"], ["cb", "ca"], ["ca", "cc"], ["ca", "cb", "cc"], ["cc", "cb", "ca"], ["cd", "ce"], ["ca", "cd", "ce"], ["ca", "cb", "cc", "cd"],
                  ["ce", "cc", "cb", "ca", "cd"], ["f1", "ca"], ["cb", "f2", "cc"]):
        for win in (len(terms), len(terms) + 1, len(terms) + 3, 12):
            if win in (len(terms), len(terms) + 3) and len(terms) <= 3:
                qs.append(dict(op="NEAR", terms=terms, first=0, maxitems=2000, window=win))      # the whole match
            qs.append(dict(op="NEAR", terms=terms, first=0, maxitems=10, window=win))
    return qs


# ---- oracle over postings copied back from a device-resident index (config-scale parity, bench cpu_baseline) ----

class DeviceOracle:
    """A CPU-oracle index over the postings of `terms` as the DEVICE holds them (decoded by K1 on the GPU and copied
    back, with the positions when `positions`), so that the oracle answers on exactly the index the HIP path
    searches — at any size, without re-inverting the corpus on the host.  Same interface as Corpus for
    oracle_search / oracle_search_batch (oracle_index())."""

    def __init__(self, db, terms, positions=False):
        from xapiand_amd import _lib
        L = _lib.lib()
        info = db.info()
        terms = sorted({t if isinstance(t, bytes) else t.encode() for t in terms})
        u32p = C.POINTER(C.c_uint32)
        self.doclen = np.zeros(info.lastdocid + 1, dtype=np.uint32)
        _lib.check(min(0, L.xgm_debug_read_doclen(db._h, self.doclen.ctypes.data_as(u32p), self.doclen.size)))
        dids, wdfs, poss, keep = [], [], [], []
        for t in terms:
            tid, tf = C.c_uint32(), C.c_uint32()
            _lib.check(L.xgm_lookup_term(db._h, t, len(t), C.byref(tid), C.byref(tf), None, None))
            if tf.value == 0:
                continue
            d = np.zeros(tf.value, dtype=np.uint32)
            w = np.zeros(tf.value, dtype=np.uint32)
            n = L.xgm_debug_decode_term_device(db._h, tid.value, d.ctypes.data_as(u32p), w.ctypes.data_as(u32p), tf.value)
            assert n == tf.value, L.xgm_last_error()
            if positions:
                p = np.zeros(int(w.sum(dtype=np.uint64)), dtype=np.uint32)
                n = L.xgm_debug_read_positions(db._h, tid.value, p.ctypes.data_as(u32p), p.size)
                assert n == p.size, L.xgm_last_error()
                poss.append(p)
            keep.append(t); dids.append(d); wdfs.append(w)
        self.terms = keep
        self.did = np.concatenate(dids) if keep else np.zeros(0, dtype=np.uint32)
        self.wdf = np.concatenate(wdfs) if keep else np.zeros(0, dtype=np.uint32)
        self.df = np.array([d.size for d in dids], dtype=np.uint32)
        self.tlen = np.array([len(t) for t in keep], dtype=np.uint32)
        self._tarr = (C.c_char_p * len(keep))(*keep)
        pos_off_p, pos_p = None, None
        if positions:
            self.pos = np.concatenate(poss) if keep else np.zeros(1, dtype=np.uint32)
            self.pos_off = np.zeros(self.wdf.size + 1, dtype=np.uint64)
            np.cumsum(self.wdf, dtype=np.uint64, out=self.pos_off[1:])
            pos_off_p, pos_p = self.pos_off.ctypes.data_as(C.POINTER(C.c_uint64)), self.pos.ctypes.data_as(u32p)
        self._oidx = olib().xgo_index_from_raw(len(keep), info.lastdocid, info.doccount, info.total_length, self.doclen.ctypes.data_as(u32p),
                                               C.cast(self._tarr, C.POINTER(C.c_char_p)), self.tlen.ctypes.data_as(u32p),
                                               self.df.ctypes.data_as(u32p), self.did.ctypes.data_as(u32p), self.wdf.ctypes.data_as(u32p),
                                               pos_off_p, pos_p)

    def oracle_index(self):
        return self._oidx

    def warm(self):
        for t in self.terms:
            olib().xgo_index_warm(self._oidx, t, len(t))          # glass chunk encoding is index-build work

    def close(self):
        if self._oidx:
            olib().xgo_index_free(self._oidx)
            self._oidx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def oracle_search_batch(corpus, queries, first, maxitems, n_threads=None, reference_select_bug=False):
    """Every query once on n_threads host threads (oracle/xgm_oracle.cc::xgo_search_batch) → [(rows, hdr dict)]."""
    ol = olib()
    nq = len(queries)
    n_threads = n_threads or max(1, min(os.cpu_count() or 1, nq))
    flat = [(t if isinstance(t, bytes) else t.encode()) for q in queries for t in q["terms"]]
    ops = (C.c_uint32 * nq)(*[OPS[q["op"]] | (((q.get("n_required") or 1) << 8) if q["op"] in SIDED else 0) for q in queries])
    nts = (C.c_uint32 * nq)(*[len(q["terms"]) for q in queries])
    wins = (C.c_uint32 * nq)(*[q.get("window", 0) for q in queries])
    terms = (C.c_char_p * len(flat))(*flat)
    lens = (C.c_uint32 * len(flat))(*[len(t) for t in flat])
    cap = max(1, first + maxitems)
    hits = (OHit * (nq * cap))()
    hdrs = (OHdr * nq)()
    ol.xgo_search_batch.restype = C.c_int
    ol.xgo_search_batch.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                    C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                    C.POINTER(OHit), C.POINTER(OHdr)]
    rc = ol.xgo_search_batch(corpus.oracle_index(), nq, ops, nts, wins, terms, lens, first, maxitems, cap, n_threads, 1 if reference_select_bug else 0, hits, hdrs)
    assert rc == 0
    out = []
    for i in range(nq):
        h = hdrs[i]
        rows = [(hits[i * cap + j].docid, hits[i * cap + j].weight, hits[i * cap + j].subqs) for j in range(h.n_hits)]
        out.append((rows, dict(n_hits=h.n_hits, matches=h.matches, max_attained=h.max_attained, max_possible=h.max_possible, max_subqs=h.max_subqs)))
    return out


# ---- nested queries: a tree of tuples <-> the post-order token form of xapian_ref's "RPN" queries ----
#   tree := "term" | ("term", wqf) | ("AND", t, t, ...) | ("OR", ...) | ("SYN", term, ...) | ("AND_NOT", left, right...) |
#           ("AND_MAYBE", left, right...) | ("FILTER", left, right) | ("SCALE", factor, t) |
#           ("WILD", prefix, term, ...) | ("WILD_OR", prefix, term, ...): OP_WILDCARD "prefix*" with the OP_SYNONYM / OP_OR combiner; the terms
#           are its expansion — every term of the corpus under the prefix, in term order: the reference expands the prefix itself (the driver's
#           "~prefix,0,E,S" / "~prefix,0,E,O" tokens), the device and the oracle are handed the list
T_KIND = {"TERM": 0, "AND": 1, "OR": 2, "AND_NOT": 3, "AND_MAYBE": 4, "FILTER": 5, "SYN": 6, "SCALE": 7, "WILD": 8, "WILD_OR": 9}
_RPN_SIGN = {"AND": "&", "OR": "|", "SYN": "=", "AND_NOT": "-", "AND_MAYBE": "?"}
_WILD = ("WILD", "WILD_OR")


def tree_from_json(t):
    """JSON turns the tuples of a tree into lists: back to tuples (a ["term", wqf] pair stays a pair)."""
    if isinstance(t, list):
        return tuple(tree_from_json(x) for x in t)
    return t


def tree_rpn(tree):
    """Post-order token list of a tree (the query-file form)."""
    if isinstance(tree, str):
        return [tree]
    if len(tree) == 2 and isinstance(tree[1], int) and isinstance(tree[0], str) and tree[0] not in T_KIND:
        return ["%s#%d" % tree]
    op = tree[0]
    if op == "SCALE":
        return tree_rpn(tree[2]) + ["*%r" % float(tree[1])]
    if op in _WILD:
        return ["~%s,0,E,%s" % (tree[1], "S" if op == "WILD" else "O")]
    toks = [x for k in tree[1:] for x in tree_rpn(k)]
    if op == "FILTER":
        return toks + ["!"]
    return toks + ["%s%d" % (_RPN_SIGN[op], len(tree) - 1)]


def tree_program(tree):
    """(terms, wqf, ops) with ops = [(kind, arity, term index, scale)] in post-order; terms distinct, in first-use order."""
    terms, wqf, ops = [], [], []

    def walk(t):
        if isinstance(t, str) or (len(t) == 2 and isinstance(t[1], int) and t[0] not in T_KIND):
            name, w = (t, 1) if isinstance(t, str) else t
            if name in terms:
                raise ValueError("repeated term %s" % name)
            terms.append(name); wqf.append(w)
            ops.append((T_KIND["TERM"], 0, len(terms) - 1, 1.0))
            return
        op = t[0]
        if op == "SCALE":
            walk(t[2])
            ops.append((T_KIND["SCALE"], 1, 0, float(t[1])))
            return
        kids = t[2:] if op in _WILD else t[1:]
        for k in kids:
            walk(k)
        ops.append((T_KIND[op], len(kids), 0, 1.0))
    walk(tree)
    return terms, wqf, ops


def oracle_search_tree(corpus, tree, first, maxitems, global_stats=None):
    """The CPU oracle on a nested query.  Returns (rows, hdr, total_subqs)."""
    ol = olib()
    terms, wqf, ops = tree_program(tree)
    tb = [t.encode() for t in terms]
    n = len(tb)
    arr = (C.c_char_p * n)(*tb)
    lens = (C.c_uint32 * n)(*[len(t) for t in tb])
    wq = (C.c_uint32 * n)(*wqf)
    m = len(ops)
    kind = (C.c_uint8 * m)(*[o[0] for o in ops])
    arity = (C.c_uint8 * m)(*[o[1] for o in ops])
    tix = (C.c_uint16 * m)(*[o[2] for o in ops])
    scale = (C.c_double * m)(*[o[3] for o in ops])
    cap = max(1, first + maxitems)
    hits = (OHit * cap)()
    hdr = OHdr()
    tot = C.c_uint32()
    ol.xgo_search_tree.restype = C.c_int
    ol.xgo_search_tree.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32,
                                   C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(C.c_uint16), C.POINTER(C.c_double), C.c_uint32, C.c_uint32,
                                   C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(OHit), C.POINTER(OHdr), C.POINTER(C.c_uint32)]
    if global_stats is None:
        rc = ol.xgo_search_tree(corpus.oracle_index(), n, arr, lens, wq, m, kind, arity, tix, scale, first, maxitems, 0, 0, 0, None, hits, C.byref(hdr), C.byref(tot))
    else:
        tf = (C.c_uint32 * n)(*[global_stats["termfreq"][t] for t in terms])
        rc = ol.xgo_search_tree(corpus.oracle_index(), n, arr, lens, wq, m, kind, arity, tix, scale, first, maxitems, 1,
                                global_stats["total_length"], global_stats["collection_size"], tf, hits, C.byref(hdr), C.byref(tot))
    assert rc == 0, rc
    return [(hits[i].docid, hits[i].weight, hits[i].subqs) for i in range(hdr.n_hits)], hdr, tot.value


def gen_tree_queries(n_queries, rank_lo=1, rank_hi=300, seed=QUERY_SEED):
    """Random nested queries over distinct terms: the shapes Xapiand's DSL builds (boolean combinations, _filter / _and_not /
    _and_maybe around them, synonym groups from wildcards, boosts)."""
    rng = random.Random(seed)

    def terms(k, used):
        out = []
        while len(out) < k:
            t = "t%d" % max(1, log_uniform_rank(rng, rank_lo, rank_hi))
            if t not in used:
                used.add(t); out.append(t)
        return out
    qs = []
    for i in range(n_queries):
        used = set()
        shape = i % 12
        a = terms(8, used)
        if shape == 0:
            tree = ("AND", ("OR", a[0], a[1]), a[2])
        elif shape == 1:
            tree = ("OR", ("AND", a[0], a[1]), a[2], ("AND", a[3], a[4]))
        elif shape == 2:
            tree = ("AND", ("OR", a[0], a[1], a[2]), ("OR", a[3], a[4]), a[5])
        elif shape == 3:
            tree = ("AND_NOT", ("OR", a[0], a[1]), ("AND", a[2], a[3]))
        elif shape == 4:
            tree = ("AND_MAYBE", ("AND", a[0], a[1]), ("OR", a[2], ("AND", a[3], a[4])))
        elif shape == 5:
            tree = ("FILTER", ("OR", a[0], a[1], a[2]), ("OR", a[3], a[4]))
        elif shape == 6:
            tree = ("OR", ("SYN", a[0], a[1], a[2]), a[3])
        elif shape == 7:
            tree = ("AND", ("SYN", a[0], a[1]), ("SCALE", 2.5, a[2]), (a[3], 3))
        elif shape == 8:
            tree = ("SCALE", 0.5, ("OR", a[0], ("SCALE", 3.0, ("AND", a[1], a[2])), a[3]))
        elif shape == 9:
            tree = ("AND", ("AND", a[0], ("OR", a[1], a[2])), ("FILTER", a[3], ("OR", a[4], a[5])))
        elif shape == 10:
            tree = ("OR", ("AND_NOT", a[0], a[1]), ("AND_MAYBE", a[2], a[3]), (a[4], 2))
        else:
            tree = ("AND_MAYBE", ("SYN", a[0], a[1]), ("SYN", a[2], a[3], a[4]), a[5])
        qs.append(dict(op="RPN", tree=tree, terms=tree_rpn(tree), first=0, maxitems=10, window=0))
    return qs


def tree_percentages(page, hdr, total_subqs):
    """MSet::convert_to_percent over the rows of a page, with percent_scale_factor = matched / total weighted subqueries of the best document
    / its weight (hdr.max_subqs, hdr.max_attained: of the WHOLE match) — what the reference driver prints beside every hit of an RPN query."""
    scale = hdr.max_subqs / float(total_subqs) / hdr.max_attained * 100.0
    return [min(100, max(1, int(w * scale + 100.0 * 2.220446049250313e-16))) if w > 0 else 0 for _, w, _ in page]


# ---- nested queries at the edges of the lowering and of the node program: a crafted corpus, an explicit table of cases ----

TREE_EDGE_LASTDOCID, TREE_EDGE_GAP = 2600, (1301, 1340)          # docids 1301 .. 1340 are deleted documents
TREE_EDGE_M = ["m%d" % i for i in range(16)]
TREE_EDGE_ABSENT = ("nosuch1", "nosuch2")


def synonym_estimate(dfs, db_size):
    """TreePlanner::synonym's estimate of a group (BoolOrPostList::get_termfreq_est): the members taken for independent."""
    scale = 1.0 / db_size
    p = dfs[0] * scale
    for df in dfs[1:]:
        pi = df * scale
        p += pi - p * pi
    return int(p * db_size + 0.5)


def or_estimate(a, b, db_size):
    """est_or: OrPostList::get_termfreq_est of two children."""
    return int(a + b - (float(a) * b / db_size) + 0.5)


def tree_edge_postings(seed=0x7EE0ED6E):
    """The corpus of the nested-query edge cases: 2 560 documents at docids 1 .. 2600 with a gap of 40 deleted ones in the middle (11 stripes of
    256, 3 of 1024).  Returns (postings {term: [(did, wdf, [1 .. wdf])]}, doclen {did: length}) for ManualCorpus and write_postings_file.
      eqA eqB eqC eqD   df 96 each out of one pool of 160 documents (they overlap in part), wdf patterns of their own: ties in every order
      eqS1 eqS2, eqL    df(eqL) == the ESTIMATE of SYN(eqS1, eqS2);  eqO: df == the estimate of OR(eqA, eqB) — asserted below
      all               every document;  one: df 1 (docid 500);  first: docid 1;  last: docid 2600
      w254a w254b       wdf 254 in the two documents they share (500, 1800): their wdf bound stays 254, the group's sum is 508
      w255, w300        a wdf of 255 (in 500) and of 300 (in 1800): terms of the 16-bit tables
      m0 .. m15         forty shared documents, and 5 + 3 i of their own
      o00 .. o23        df 3 .. 1500 in geometric steps, wdf 1 .. 5
    nosuch1 / nosuch2 (TREE_EDGE_ABSENT) have no postings.  Every choice is a function of hash64: the same corpus on every Python."""
    last, gap = TREE_EDGE_LASTDOCID, TREE_EDGE_GAP
    live = [d for d in range(1, last + 1) if not gap[0] <= d <= gap[1]]
    post = {}

    def pick(tag, pool, n):
        return sorted(sorted(pool, key=lambda d: hash64(seed, tag, d))[:n])

    def put(term, docs, wdf):
        post[term] = [(d, wdf(d), list(range(1, wdf(d) + 1))) for d in docs]
    put("all", live, lambda d: 1 + d % 3)
    pool = pick(1, live, 320)
    pool_eq = pick(2, pool, 160)              # (four sets of 96 out of 160: some twenty documents hold all four)
    put("eqA", pick(10, pool_eq, 96), lambda d: 1 + d % 3)
    put("eqB", pick(11, pool_eq, 96), lambda d: 1 + d % 2)
    put("eqC", pick(12, pool_eq, 96), lambda d: 1 + (d // 3) % 3)
    put("eqD", pick(13, pool_eq, 96), lambda d: 2 if d % 5 == 0 else 1)
    put("eqS1", pick(20, pool, 64), lambda d: 1 + d % 2)
    put("eqS2", pick(21, pool, 80), lambda d: 1 + (d // 2) % 2)
    put("eqL", pick(22, pool, 142), lambda d: 1)
    put("eqO", pick(23, pool, 188), lambda d: 1)
    put("one", [500], lambda d: 3)
    put("first", [1], lambda d: 2)
    put("last", [last], lambda d: 2)
    put("w254a", [500, 1800], lambda d: 254)
    put("w254b", [500, 1800], lambda d: 254)
    put("w255", [500, 1900], lambda d: 255 if d == 500 else 7)
    put("w300", [640, 1800], lambda d: 300 if d == 1800 else 2)
    shared = [100 + 60 * j for j in range(40)]
    assert not any(gap[0] <= d <= gap[1] for d in shared)
    rest = [d for d in live if d not in shared]
    for i, m in enumerate(TREE_EDGE_M):
        put(m, sorted(shared + pick(40 + i, rest, 5 + 3 * i)), lambda d, i=i: 1 + (d + i) % 2)
    for i in range(24):
        put("o%02d" % i, pick(100 + i, live, int(round(3 * 500 ** (i / 23.0)))), lambda d, i=i: 1 + hash64(seed, 200 + i, d) % 5)
    doclen = {d: 0 for d in live}
    for pl in post.values():
        for d, w, _ in pl:
            doclen[d] += w
    db_size = len(live)
    assert db_size == 2560 and len(post["all"]) == db_size and not set(TREE_EDGE_ABSENT) & set(post)
    # the ties the cases rest on: equal df, and a leaf whose df IS a sub-tree's estimate
    assert len({len(post[t]) for t in ("eqA", "eqB", "eqC", "eqD")}) == 1
    assert len(post["eqL"]) == synonym_estimate([len(post["eqS1"]), len(post["eqS2"])], db_size) == synonym_estimate([len(post["eqS2"]), len(post["eqS1"])], db_size)
    assert len(post["eqO"]) == or_estimate(len(post["eqA"]), len(post["eqB"]), db_size)
    return post, doclen


def tree_edge_prefix(prefix):
    """The expansion of "prefix*" over the crafted corpus, in term order (the terms are fixed names: no corpus is built for this)."""
    names = (["all", "one", "first", "last", "eqA", "eqB", "eqC", "eqD", "eqS1", "eqS2", "eqL", "eqO", "w254a", "w254b", "w255", "w300"] + TREE_EDGE_M +
             ["o%02d" % i for i in range(24)])
    return sorted(t for t in names if t.startswith(prefix))


def tree_edge_cases():
    """[(name, tree)]: the nested queries at the edges of plan_tree's lowering and of the match kernel's node program, on tree_edge_postings().
    The name's first word says which edge: tie (equal estimates), root (the root is a group), one (AND / OR of one child), flat (the flattening
    rules), sided (AND_NOT / AND_MAYBE with several right-hand children), absent (terms the shard does not hold), all (a term in every
    document), width (synonym groups at the wdf tables' width), limit (16 terms, 40 ops), wild (OP_WILDCARD), quirk (an OR over AND_NOT /
    AND_MAYBE children: where the reference may lose documents)."""
    A, B, C, D, S1, S2, L, O = "eqA", "eqB", "eqC", "eqD", "eqS1", "eqS2", "eqL", "eqO"
    N1, N2 = TREE_EDGE_ABSENT
    M = TREE_EDGE_M
    W = lambda kind, prefix: (kind, prefix) + tuple(tree_edge_prefix(prefix))
    chain = M[0]
    for i in range(1, 16):                    # 16 terms + 15 AND_MAYBE + 9 SCALE = 40 ops: the longest program
        chain = ("AND_MAYBE", chain, ("SCALE", 1.0 + i / 8.0, M[i]) if i <= 9 else M[i])
    cases = [
        # -- equal estimates: MultiAnd's partial_sort_copy and the OR heap among leaves of one df, every which way
        ("tie_and_abcd", ("AND", A, B, C, D)), ("tie_and_dcba", ("AND", D, C, B, A)), ("tie_and_bdac", ("AND", B, D, A, C)),
        ("tie_and_cab", ("AND", C, A, B)),
        ("tie_or_abcd", ("OR", A, B, C, D)), ("tie_or_dcba", ("OR", D, C, B, A)), ("tie_or_cadb", ("OR", C, A, D, B)),
        ("tie_or_with_others", ("OR", A, "o10", B, "o05", C, D, "o14")),
        ("tie_and_with_others", ("AND", "o22", A, "o23", B, "all", C)),
        ("tie_and_syn_leaf", ("AND", ("SYN", S1, S2), L)), ("tie_and_leaf_syn", ("AND", L, ("SYN", S2, S1))),
        ("tie_or_syn_leaf", ("OR", ("SYN", S1, S2), L, A)), ("tie_or_leaf_syn", ("OR", A, L, ("SYN", S1, S2))),
        ("tie_and_leaf_or", ("AND", O, ("OR", A, B))), ("tie_and_or_leaf", ("AND", ("OR", B, A), O)),
        ("tie_or_scaled", ("OR", ("SCALE", 2.0, A), B, ("SCALE", 0.5, C), (D, 3))),
        ("tie_maybe_right", ("AND_MAYBE", "o20", A, B, C, D)), ("tie_andnot_right", ("AND_NOT", "all", C, A, B)),
        # -- the root is a group: tree_len == 0
        ("root_term", "o12"), ("root_term_wqf", ("o12", 3)), ("root_scale", ("SCALE", 2.5, "o12")), ("root_scale_scale", ("SCALE", 2.0, ("SCALE", 0.25, A))),
        ("root_syn", ("SYN", A, B)), ("root_syn_of_one", ("SYN", ("o12", 2))),
        # -- AND / OR of one child is that child
        ("one_and", ("AND", "o12")), ("one_or_of_and", ("OR", ("AND", A, B))), ("one_and_of_or_of_one", ("AND", ("OR", "o05"))),
        ("one_inside", ("AND", ("OR", ("AND", "o20")), ("AND", ("OR", "o21", "o19")))),
        # -- flattening
        ("flat_filter_in_and", ("AND", A, ("FILTER", B, C))), ("flat_filters_in_and", ("AND", ("FILTER", "o23", "o21"), "o22", ("FILTER", "all", "o20"))),
        ("flat_filter_of_filter_left", ("FILTER", ("FILTER", A, B), C)), ("flat_filter_of_filter_right", ("FILTER", A, ("FILTER", B, C))),
        ("flat_or_scale_in_or", ("OR", A, ("SCALE", 2.0, ("OR", B, C)), D)), ("flat_or_scale_in_or_2", ("OR", "o08", ("SCALE", 0.5, ("OR", "o09", "o10")), "o07")),
        ("flat_maybe_zero_in_filter", ("FILTER", A, ("AND_MAYBE", B, C))), ("flat_maybe_zero_in_andnot", ("AND_NOT", "o20", ("AND_MAYBE", A, B))),
        ("flat_maybe_zero_deep", ("AND", "o20", ("FILTER", "o19", ("AND_MAYBE", "o18", "o03", "o04")))),
        # -- AND_NOT / AND_MAYBE with several right-hand children
        ("sided_andnot_or_and", ("AND_NOT", "o22", "o10", ("OR", "o11", "o12"), ("AND", "o20", "o21"))),
        ("sided_maybe_or_and", ("AND_MAYBE", "o20", "o10", ("OR", A, B), ("AND", "o21", "o22"))),
        ("sided_andnot_of_andnot", ("AND_NOT", ("AND_NOT", "o23", "o20"), "o21")), ("sided_andnot_under_andnot", ("AND_NOT", "o23", ("AND_NOT", "o20", "o21"))),
        ("sided_andnot_many", ("AND_NOT", "all", "o18", "o19", ("OR", "o16", ("OR", "o17", "o15")))),
        # -- absent terms, at every position
        ("absent_root", N1), ("absent_and", ("AND", A, N1)), ("absent_or", ("OR", A, N1, B)), ("absent_or_all", ("OR", N1, N2)),
        ("absent_syn", ("SYN", A, N1)), ("absent_syn_all", ("SYN", N1, N2)), ("absent_syn_in_and", ("AND", ("SYN", N1, "o20"), "o21")),
        ("absent_andnot_right", ("AND_NOT", A, N1)), ("absent_andnot_left", ("AND_NOT", N1, A)),
        ("absent_maybe_right", ("AND_MAYBE", A, N1)), ("absent_maybe_left", ("AND_MAYBE", N1, A)),
        ("absent_filter_right", ("FILTER", A, N1)), ("absent_filter_left", ("FILTER", N1, A)),
        ("absent_deep", ("OR", ("AND", N1, "o20"), ("AND_MAYBE", "o12", N2), "o03")),
        # (a WEIGHTED synonym none of whose members the shard holds is no postlist at all, LocalSubMatch::make_synonym_postlist: an OR drops it —
        #  another Huffman tree, another max_possible —, an AND with it is nothing and lowers no further subquery: total_subqs, the percentages.
        #  The group comes LAST in lowering order in each of these: see tree_edge_unpinned_cases)
        ("absent_syn_all_in_or", ("OR", A, B, C, ("SYN", N1, N2))), ("absent_syn_all_scaled", ("OR", A, "o12", ("SCALE", 2.0, ("SYN", N2, N1)))),
        ("absent_syn_all_in_and_in_or", ("OR", "o12", ("AND", "o22", ("SYN", N1, N2), "o20", "o21"))),
        ("absent_syn_all_maybe_right", ("AND_MAYBE", A, ("SYN", N1, N2))), ("absent_syn_all_maybe_left", ("OR", "o12", ("AND_MAYBE", ("SYN", N1, N2), "o20"))),
        ("absent_syn_all_filter_right", ("FILTER", A, ("SYN", N1, N2))), ("absent_syn_all_filter_left", ("OR", "o12", ("FILTER", ("SYN", N1, N2), "o20"))),
        ("absent_syn_all_andnot_right", ("AND_NOT", A, ("SYN", N1, N2))), ("absent_syn_all_andnot_left", ("OR", "o12", ("AND_NOT", ("SYN", N1, N2), "o20"))),
        # -- a term in every document: est == db_size, AND_NOT's estimate 0
        ("all_and", ("AND", "all", A)), ("all_andnot_right", ("AND_NOT", A, "all")), ("all_andnot_left", ("AND_NOT", "all", A)),
        ("all_or", ("OR", "all", "one")), ("all_maybe", ("AND_MAYBE", "all", "first", "last")),
        ("all_zero_estimates_tie", ("AND", ("AND_NOT", A, "all"), N1, B)), ("all_filter", ("FILTER", "o05", "all")),
        # -- synonym groups at the wdf tables' width
        ("width_syn_508", ("SYN", "w254a", "w254b")), ("width_syn_508_in_or", ("OR", ("SYN", "w254a", "w254b"), "one", "first", "last")),
        ("width_syn_508_in_and", ("AND", ("SYN", "w254b", "w254a"), "one")), ("width_syn_255", ("SYN", "w254a", "w255")),
        ("width_syn_808", ("SYN", "w254a", "w254b", "w300")), ("width_or_wide_syn", ("OR", ("SYN", "w255", "w300"), A)),
        # -- the size limits
        ("limit_and16", ("AND",) + tuple(M)), ("limit_or16", ("OR",) + tuple(M)),
        ("limit_and_syn8", ("AND",) + tuple(("SYN", M[2 * i], M[2 * i + 1]) for i in range(8))),
        ("limit_or_syn8", ("OR",) + tuple(("SYN", M[2 * i + 1], M[2 * i]) for i in range(8))),
        ("limit_prog40", chain),
        # -- OP_WILDCARD over the crafted prefixes
        ("wild_root_eq", W("WILD", "eq")), ("wild_or_root_eq", W("WILD_OR", "eq")), ("wild_m", W("WILD", "m")), ("wild_or_m", W("WILD_OR", "m")),
        ("wild_w25_in_and", ("AND", W("WILD", "w25"), "all")), ("wild_or_in_or", ("OR", A, W("WILD_OR", "w25"), "o10")),
        ("wild_of_one", W("WILD", "fir")), ("wild_or_of_one", ("AND_MAYBE", "all", W("WILD_OR", "las"))),
        # -- an OR over AND_NOT / AND_MAYBE children
        ("quirk_or_sided", ("OR", ("AND_NOT", A, B), ("AND_MAYBE", C, D), ("o12", 2))), ("quirk_or_andnot", ("OR", ("AND_NOT", "o20", "o21"), "o05")),
        ("quirk_or_maybe", ("OR", ("AND_MAYBE", "o10", "o22"), ("AND_MAYBE", "o11", "o23"))),
    ]
    assert len({n for n, _ in cases}) == len(cases)
    assert len(tree_program(chain)[2]) == 40
    return cases


def tree_edge_unpinned_cases():
    """[(name, tree)]: an all-absent weighted synonym group with a term lowered AFTER it.  The compiled reference cannot pin these: it deletes the
    group's OR together with the leaf postlist its optimiser keeps as a hint (localsubmatch.cc:205-209, 273-279) and opens the next term through the
    dangling pointer — it crashes.  The oracle and the device lower them by the rule the reference's code states; they are compared with each other."""
    A, B, C = "eqA", "eqB", "eqC"
    N1, N2 = TREE_EDGE_ABSENT
    return [("unpinned_syn_all_first_in_or", ("OR", ("SYN", N1, N2), A, B, C)), ("unpinned_syn_all_scaled", ("OR", A, ("SCALE", 2.0, ("SYN", N2, N1)), "o12")),
            ("unpinned_syn_all_in_and_in_or", ("OR", ("AND", "o22", ("SYN", N1, N2), "o20", "o21"), "o12")),
            ("unpinned_syn_all_maybe_left", ("OR", ("AND_MAYBE", ("SYN", N1, N2), "o20"), "o12"))]


def tree_has_or_over_sided(tree):
    """Whether a tree holds an OR with an AND_NOT / AND_MAYBE child — the only shape that may be flagged as the reference's quirk."""
    if isinstance(tree, str) or tree[0] not in T_KIND:
        return False
    kids = [k for k in (tree[2:] if tree[0] in _WILD + ("SCALE",) else tree[1:]) if not isinstance(k, str)]
    if tree[0] == "OR" and any(k[0] in ("AND_NOT", "AND_MAYBE") for k in kids):
        return True
    return any(tree_has_or_over_sided(k) for k in kids)


def tree_edge_queries(cases=None, first=0, maxitems=10):
    return [dict(op="RPN", name=n, tree=t, terms=tree_rpn(t), first=first, maxitems=maxitems, window=0) for n, t in (cases or tree_edge_cases())]


def tree_edge_declined():
    """[dict(name, terms, ops, want, n_terms, n_tree)]: programs xgm_plan_query must refuse, with the outcome plan_tree gives each: "UNSUPPORTED"
    (a shape the device does not take: the CPU matcher's) or "INVALID" (a program no Query builds).  ops = [(kind, arity, term, scale)] as
    tree_program makes them; n_terms / n_tree, where given, overrule the lengths (17 terms and 41 ops do not fit the descriptor's arrays: the
    planner refuses by the counts alone)."""
    K = T_KIND
    T = lambda i: (K["TERM"], 0, i, 1.0)
    prog = lambda tree: tree_program(tree)
    out = []

    def add(name, want, terms, ops, **kw):
        out.append(dict(name=name, want=want, terms=list(terms), ops=list(ops), n_terms=kw.get("n_terms", len(terms)), n_tree=kw.get("n_tree", len(ops))))
    t16, _, o16 = prog(("AND",) + tuple(TREE_EDGE_M))
    add("terms_17", "UNSUPPORTED", t16, o16, n_terms=17)
    chain = dict(tree_edge_cases())["limit_prog40"]
    t40, _, o40 = prog(chain)
    add("ops_41", "UNSUPPORTED", t40, o40, n_tree=41)
    add("ops_0", "UNSUPPORTED", ["eqA"], [], n_tree=0)
    for name, f in (("scale_zero", 0.0), ("scale_negative", -1.5), ("scale_nan", float("nan"))):
        add(name, "UNSUPPORTED", ["eqA"], [T(0), (K["SCALE"], 1, 0, f)])
    add("term_index_twice", "UNSUPPORTED", ["eqA", "eqB"], [T(0), T(0), (K["AND"], 2, 0, 1.0)])
    add("term_bytes_twice", "UNSUPPORTED", ["eqA", "eqA"], [T(0), T(1), (K["OR"], 2, 0, 1.0)])
    add("term_index_out_of_range", "UNSUPPORTED", ["eqA", "eqB"], [T(0), T(2), (K["AND"], 2, 0, 1.0)])
    add("term_unused", "UNSUPPORTED", ["eqA", "eqB", "eqC"], [T(0), T(1), (K["AND"], 2, 0, 1.0)])
    add("syn_over_and", "UNSUPPORTED", ["eqA", "eqB", "eqC"], [T(0), T(1), (K["AND"], 2, 0, 1.0), T(2), (K["SYN"], 2, 0, 1.0)])
    add("wild_over_scale", "UNSUPPORTED", ["eqA", "eqB"], [T(0), (K["SCALE"], 1, 0, 2.0), T(1), (K["WILD"], 2, 0, 1.0)])
    add("wild_or_over_or", "UNSUPPORTED", ["eqA", "eqB", "eqC"], [T(0), T(1), (K["OR"], 2, 0, 1.0), T(2), (K["WILD_OR"], 2, 0, 1.0)])
    add("arity_0", "INVALID", ["eqA"], [T(0), (K["AND"], 0, 0, 1.0)])
    add("arity_beyond_stack", "INVALID", ["eqA", "eqB"], [T(0), T(1), (K["OR"], 3, 0, 1.0)])
    add("operator_first", "INVALID", ["eqA"], [(K["SCALE"], 1, 0, 2.0), T(0)])
    add("filter_of_3", "INVALID", ["eqA", "eqB", "eqC"], [T(0), T(1), T(2), (K["FILTER"], 3, 0, 1.0)])
    add("filter_of_1", "INVALID", ["eqA"], [T(0), (K["FILTER"], 1, 0, 1.0)])
    add("andnot_of_1", "INVALID", ["eqA"], [T(0), (K["AND_NOT"], 1, 0, 1.0)])
    add("maybe_of_1", "INVALID", ["eqA"], [T(0), (K["AND_MAYBE"], 1, 0, 1.0)])
    add("two_roots", "INVALID", ["eqA", "eqB"], [T(0), T(1)])
    add("unknown_kind", "INVALID", ["eqA", "eqB"], [T(0), T(1), (10, 2, 0, 1.0)])
    return out


# ---- the positional filter (PHRASE, windowed PHRASE, NEAR) at its edges: a crafted corpus, an explicit table of cases ----
#
# The corpus is made of GROUPS.  A group is a run of at most 64 consecutive docids inside one stripe of 256, and a set of terms of its own:
# every document of the group holds every term of the group, nothing else does — the conjunction of a case IS its group, whatever the
# positions say.  A term of a "dense" flavour also stands (once, wdf 1) in some 480 - 510 of the filler documents 1 .. 2048, in a residue
# class of its own, so that it has probe containers (32 postings per stripe on average) while no filler document holds two terms of one
# group; a rare term has a flat posting array.  How many filler documents a term stands in fixes the plan order (ascending termfreq).

POS_EDGE_LASTDOCID, POS_EDGE_FILL, POS_EDGE_SEED = 3839, 2048, 0x9051ED6E
POS_EDGE_MAXITEMS, POS_EDGE_MAX_CONJ = 192, 150
POS_EDGE_FLAVOUR_STEP = 16400            # a group's documents carry the same lists once per flavour, this far apart (four flavours stay 2-byte)
LEN16 = (1, 4, 5, 8, 9, 16, 17, 32, 33, 48, 49, 64, 65, 128, 254)          # list lengths of a term, 2-byte lists: fast | wide | serial
LEN32 = (1, 4, 5, 16, 17, 64, 65, 252, 253, 254)                            # ... 4-byte lists
DECISIVE = (0, 7, 8, 15, 16, 31, 32, 47, 48, 63, 64)                        # where in the long list the deciding position sits (and n - 1)


class _Cur:
    """A PositionList over a sorted list: next / skip_to / get_position, forward only."""

    def __init__(self, pp):
        self.p, self.c = pp, -1

    def next(self):
        self.c += 1
        return self.c < len(self.p)

    def skip_to(self, want):
        if self.c < 0:
            self.c = 0
        while self.c < len(self.p) and self.p[self.c] < want:
            self.c += 1
        return self.c < len(self.p)

    def get(self):
        return self.p[self.c]


def py_phrase_exact(lists):
    """ExactPhrasePostList::test_doc (exactphrasepostlist.cc:75-133) on the lists in PHRASE order."""
    n = len(lists)
    order = sorted(range(n), key=lambda i: len(lists[i]))              # by wdf; a stable sort, as std::sort is on so few
    pl = [_Cur(lists[i]) for i in order]
    if not pl[0].skip_to(order[0]):
        return False
    if len(pl[0].p) > len(pl[1].p):
        if not pl[1].skip_to(order[1]):
            return False
        pl[0], pl[1] = pl[1], pl[0]
        order[0], order[1] = order[1], order[0]
    idx0 = order[0]
    base = pl[0].get() - idx0
    i = 1
    while True:
        required = base + order[i]
        if not pl[i].skip_to(required):
            return False
        got = pl[i].get()
        if got == required:
            i += 1
            if i == n:
                return True
            continue
        if not pl[0].skip_to(got - order[i] + idx0):
            return False
        base = pl[0].get() - idx0
        i = 1


def py_phrase_window(lists, window):
    """PhrasePostList::test_doc (phrasepostlist.cc:60-90) on the lists in PHRASE order."""
    n = len(lists)
    pl = [_Cur(pp) for pp in lists]
    if not pl[0].next():
        return False
    while True:
        base = pos = pl[0].get()
        i = 0
        while True:
            i += 1
            if i == n:
                return True
            if not pl[i].skip_to(pos + 1):
                return False
            pos = pl[i].get()
            b = pos + (n - i)
            if not b - base <= window:
                break
        if not pl[0].skip_to(b - window):
            return False


def py_near(lists, window):
    """NearPostList::test_doc (nearpostlist.cc:60-160) for lists that share no position: started lazily in ascending wdf order, the smallest
    head skipped to last - window + 1 while the span is too wide.  The duplicate-position walk (lines 106-140) finds nothing to move."""
    order = sorted(range(len(lists)), key=lambda i: len(lists[i]))
    heads = [_Cur(lists[order[0]])]
    if not heads[0].next():
        return False
    last = heads[0].get()
    while True:
        top = min(heads, key=lambda c: c.get())
        if last - top.get() < window:
            if len(heads) != len(lists):
                c = _Cur(lists[order[len(heads)]])
                if last < window:
                    if not c.next():
                        return False
                elif not c.skip_to(last - window + 1):
                    return False
                last = max(last, c.get())
                heads.append(c)
                continue
            assert len({c.get() for c in heads}) == len(heads)
            return True
        if not top.skip_to(last - window + 1):
            return False
        last = max(last, top.get())


def py_positional(op, lists, window):
    """The verdict of the reference's procedures on one document; lists in query order, window 0 = the number of terms."""
    n = len(lists)
    w = window or n
    if op == "NEAR":
        return py_near(lists, w)
    return py_phrase_exact(lists) if w == n else py_phrase_window(lists, w)


def full_search_positional(op, lists, window):
    """What the procedures are FOR, by exhaustive search: PHRASE — positions p_0 < p_1 < ... in phrase order with p_i + (n - i) - p_0 <= window
    for every i >= 1 (window == n: p_i = p_0 + i); NEAR — one position of every term inside a span shorter than the window."""
    n = len(lists)
    w = window or n
    if op == "NEAR":
        return any(all(any(x <= p < x + w for p in pp) for pp in lists) for x in set().union(*lists))
    if w == n:
        sets = [set(pp) for pp in lists]
        return any(all(b + i in sets[i] for i in range(n)) for b in lists[0])

    def chain(i, prev, base):
        return i == n or any(chain(i + 1, p, base) for p in lists[i] if p > prev and p + (n - i) - base <= w)
    return any(chain(1, b, b) for b in lists[0])


def _craft_lists(op, window, T, p_long, n, idx, match, stride=64):
    """T lists in query order: list p_long has n entries `stride` apart, every other list one entry, placed so that entry idx of the long
    list decides — a match, or (match False) the near-miss: one deciding position moved by one."""
    w = window or T
    assert stride > w + T and 0 <= idx < n
    L = [16 + T + stride * m for m in range(n)]
    x = L[idx]
    lists = [None] * T
    lists[p_long] = L
    others = [j for j in range(T) if j != p_long]
    if op == "NEAR":                                  # the others next to x, the last of them at the far end of the window
        for k, j in enumerate(others[:-1]):
            lists[j] = [x + 1 + k]
        lists[others[-1]] = [x + w - 1 + (0 if match else 1)]
    elif w == T:                                      # exact: word j at base + j; the near-miss moves an outer word outwards
        for j in others:
            lists[j] = [x - p_long + j]
        if not match:
            q = others[-1] if others[-1] > p_long else others[0]
            lists[q] = [lists[q][0] + (1 if q > p_long else -1)]
    else:                                             # windowed: words 0 .. T-2 side by side, the last one window - 1 after the first (or window)
        far = w - 1 + (0 if match else 1)
        base = x - (far if p_long == T - 1 else p_long)
        for j in others:
            lists[j] = [base + (far if j == T - 1 else j)]
    return lists


class _PosEdgeBuilder:
    def __init__(self):
        self.rng = random.Random(POS_EDGE_SEED)
        self.post, self.doclen, self.next_doc = {}, {}, POS_EDGE_FILL + 1
        self.fill_pos = {}
        self.cases, self.intent, self.term_info, self.groups = [], {}, {}, {}

    def _put(self, term, d, pp):
        pp = sorted(pp)
        assert len(set(pp)) == len(pp) and pp
        self.post.setdefault(term, []).append((d, len(pp), pp))
        self.doclen[d] = self.doclen.get(d, 0) + len(pp)

    def term(self, name, j, extras, wide=False):
        """A term standing `extras` times in the filler documents of residue class j % 4 (rare terms of long queries: their own stretch of it)."""
        cls = [d for d in range(1, POS_EDGE_FILL + 1) if d % 4 == j % 4]
        assert extras <= len(cls) - 120 * (j // 4)
        for d in cls[120 * (j // 4):120 * (j // 4) + extras]:
            p = self.fill_pos.get(d, 0) + 1
            self.fill_pos[d] = p
            self._put(name, d, [p])
        self.term_info[name] = dict(dense=extras >= 480, wide=wide, extras=extras)

    def group(self, name, T, docs, flavours, share=None):
        """docs: [lists in query order]; flavours: {tag: (extras per term, position offset)}; share: {tag: family} — the terms of that flavour are the
        family's, which several groups hold (a conjunction of more than 64 documents).  Returns {tag: [terms]} and the docids."""
        n = len(docs)
        assert n <= 64
        if (self.next_doc - 1) % 256 + n > 256:
            self.next_doc = ((self.next_doc - 1) // 256 + 1) * 256 + 1
        dids = list(range(self.next_doc, self.next_doc + n))
        self.next_doc += n
        assert self.next_doc - 1 <= POS_EDGE_LASTDOCID
        terms = {}
        for tag, (extras, off) in flavours.items():
            names = ["%s%s%s" % ((share or {}).get(tag, name), tag, "abcdefgh"[j]) for j in range(T)]
            wide = [any(p + off >= 65536 for lists in docs for p in lists[j]) for j in range(T)]
            for j, t in enumerate(names):
                if t not in self.term_info:
                    self.term(t, j, extras[j], wide[j])
                assert self.term_info[t]["wide"] == wide[j]
                for d, lists in zip(dids, docs):
                    self._put(t, d, [p + off for p in lists[j]])
            terms[tag] = names
        self.groups[name] = dict(dids=dids, docs=docs, terms=terms, offs={tag: off for tag, (_, off) in flavours.items()})
        return terms, dids

    def case(self, name, op, terms, window, group, perm=None, aimed=()):
        """A table entry.  perm: the query's terms are the group's in this order (the lists follow).  aimed: [(index of the group's document,
        intended verdict)] — the documents crafted for this very case."""
        self.cases.append(dict(name=name, edge=name.split("_")[0], op=op, terms=list(terms), window=window, group=group, perm=list(perm) if perm else None,
                               first=0, maxitems=POS_EDGE_MAXITEMS))
        for i, v in aimed:
            self.intent[(name, self.groups[group]["dids"][i])] = v


D2, F2, R2 = (484, 500), (0, 500), (0, 6)                      # two terms: both with containers | a rare leader | both rare
_FL2 = {"d": (D2, 0), "f": (F2, POS_EDGE_FLAVOUR_STEP), "r": (R2, 2 * POS_EDGE_FLAVOUR_STEP)}
_OPS3 = (("ex", "PHRASE", 0), ("win", "PHRASE", 3), ("near", "NEAR", 2))        # tag, op, window - number of terms (0: exact)
_X8 = (10, 2, 14, 6, 0, 12, 4, 8)                             # filler postings of a rare term by its place in the query: plan order != query order


def _win(T, extra):
    return T + extra if extra else 0


_pos_edge_cache = None


def _positional_edges():
    global _pos_edge_cache
    if _pos_edge_cache is not None:
        return _pos_edge_cache
    B = _PosEdgeBuilder()
    rng = B.rng

    def two(edge, gname, tag, op, window, docs, aimed, flavours=_FL2, share=None):
        """A two-term group in its flavours, asked in both query orders where the order is free (NEAR)."""
        terms, _ = B.group(gname, 2, docs, flavours, share)
        for fl, names in terms.items():
            if fl in (share or {}):
                continue
            B.case("%s_%s%s_%s" % (edge, gname, fl, tag), op, names, window, gname, aimed=aimed)
            if op == "NEAR":
                B.case("%s_%s%s_%s_rev" % (edge, gname, fl, tag), op, names[::-1], window, gname, perm=[1, 0], aimed=aimed)

    # -- len: the length of a term's list, 2-byte lists; the deciding entry is the list's last; the long list under plan term 0 (a) and under the last (b)
    for tag, op, extra in _OPS3:
        docs, aimed = [], []
        for n in LEN16:
            for p_long in (0, 1):
                for match in (True, False):
                    docs.append(_craft_lists(op, _win(2, extra), 2, p_long, n, n - 1, match))
                    aimed.append((len(docs) - 1, match))
        two("len", "l" + tag, tag, op, _win(2, extra), docs, aimed)
    # -- len4: 4-byte lists (every position past 65 535).  The exact group's terms sort last and its last document is the 254-entry list whose
    #    match is its last entry: the last list of the positions section
    for tag, op, extra in _OPS3:
        docs, aimed = [], []
        for n in LEN32:
            for p_long in (0, 1):
                for match in (False, True):
                    docs.append([[p + 66000 for p in pp] for pp in _craft_lists(op, _win(2, extra), 2, p_long, n, n - 1, match)])
                    aimed.append((len(docs) - 1, match))
        gname = "zz4" if tag == "ex" else "q" + tag
        two("len4", gname, tag, op, _win(2, extra), docs, aimed, flavours={"d": (D2, 0), "r": (R2, 40000)})
    # -- idx: where in the long list the deciding entry sits: lists of 16 (fast), 64 (wide), 254 (serial)
    for gname, op, extra, p_long in (("ia", "PHRASE", 0, 0), ("ib", "PHRASE", 0, 1), ("in", "NEAR", 2, 0), ("iw", "PHRASE", 1, 1)):
        docs, aimed = [], []
        for n in (16, 64, 254):
            for idx in sorted({i for i in DECISIVE if i < n} | {n - 1}):
                for match in (True, False):
                    docs.append(_craft_lists(op, _win(2, extra), 2, p_long, n, idx, match))
                    aimed.append((len(docs) - 1, match))
        fam = gname in ("ia", "ib")
        two("idx", gname, {"PHRASE": "ex" if not extra else "win", "NEAR": "near"}[op], op, _win(2, extra), docs, aimed,
            flavours=dict(_FL2, u=(D2, 3 * POS_EDGE_FLAVOUR_STEP)) if fam else _FL2, share={"u": "iu"} if fam else None)
    # -- round: what a round of 64 survivors is made of.  f: at most 16 positions of a term, w: 17 .. 64, s: more; verdicts alternate
    kinds = {"f": (1, 2, 3, 5, 8, 9, 12, 16), "w": (17, 20, 31, 32, 33, 48, 64), "s": (65, 100, 254)}
    rounds = (("f64", "f" * 64), ("w16", "w" * 16), ("w17", "w" * 17), ("w33", "w" * 33), ("w64", "w" * 64), ("s1st", "s" + "f" * 63), ("slast", "f" * 63 + "s"),
              ("mix", "fwsfwfsw" * 8))
    for gname, comp in rounds:
        docs, aimed = [], []
        for i, k in enumerate(comp):
            n = rng.choice(kinds[k])
            docs.append(_craft_lists("PHRASE", 0, 2, i // 2 % 2, n, rng.randrange(n), i % 2 == 0))
            aimed.append((i, i % 2 == 0))
        fam = gname in ("w64", "mix")
        two("round", "r" + gname, "ex", "PHRASE", 0, docs, aimed, flavours=dict({"d": (D2, 0), "f": (F2, POS_EDGE_FLAVOUR_STEP)}, **({"v": (R2, 2 * POS_EDGE_FLAVOUR_STEP)} if fam else {})),
            share={"v": "ru"} if fam else None)
    # -- several: conjunctions of more than 64 documents (two groups that share a flavour's terms): more than one round of survivors, and at a page
    #    of ten a k-th weight that drops candidates before their positions are tested
    for fam, fl, gs in (("iu", "u", ["ia", "ib"]), ("ru", "v", ["rw64", "rmix"])):
        names = B.groups[gs[0]]["terms"][fl]
        assert names == B.groups[gs[1]]["terms"][fl]
        for tag, op, extra in _OPS3:
            B.case("several_%s%s_%s" % (fam, fl, tag), op, names, _win(2, extra), gs)
    # -- plan: the long list under plan term 0, the last, and (5 and 8 terms) plan terms 4 and 7; lists of 12 (fast), 20 (wide), 70 (serial)
    for T, flavours in ((3, ("d", "f")), (4, ("d", "f")), (5, ("r",)), (8, ("r",))):
        order = sorted(range(T), key=lambda j: _X8[j])                       # plan order: ascending termfreq
        where = sorted({0, T - 1} | ({4} if T > 4 else set()))
        docs, aimed_by = [], {}
        for tag, op, extra in _OPS3:
            for k in where:
                for n in (12, 20, 70):
                    for match in (True, False):
                        docs.append(_craft_lists(op, _win(T, extra), T, order[k], n, n - 1, match))
                        aimed_by.setdefault(tag, []).append((len(docs) - 1, match))
        fl = {}
        for f in flavours:
            ex = [_X8[j] for j in range(T)]
            if f == "d": ex = [480 + 2 * e for e in ex]
            if f == "f": ex = [0 if e == min(ex) else 480 + 2 * e for e in ex]
            fl[f] = (ex, POS_EDGE_FLAVOUR_STEP * len(fl))
        terms, _ = B.group("p%d" % T, T, docs, fl)
        for f, names in terms.items():
            for tag, op, extra in _OPS3:
                B.case("plan_p%d%s_%s" % (T, f, tag), op, names, _win(T, extra), "p%d" % T, aimed=aimed_by[tag])
    # -- width: a phrase that ends at 65 535 (both lists 2-byte), one at 65 535 / 65 536 (a 2-byte and a 4-byte term, in both plan orders)
    docs = [[[65534], [65535]], [[65533], [65535]], [[7, 65534], [9, 30, 65535]], [[7, 65533], [9, 30, 65535]]]
    terms, _ = B.group("w16", 2, docs, {"d": (D2, 0)})
    B.case("width_w16d_ex", "PHRASE", terms["d"], 0, "w16", aimed=[(0, True), (1, False), (2, True), (3, False)])
    B.case("width_w16d_near", "NEAR", terms["d"][::-1], 2, "w16", perm=[1, 0], aimed=[(0, True), (1, False), (2, True), (3, False)])
    terms, _ = B.group("w16r", 2, docs, {"r": (R2, 0)})
    B.case("width_w16r_ex", "PHRASE", terms["r"], 0, "w16r", aimed=[(0, True), (1, False), (2, True), (3, False)])
    docs = [[[65535], [65536]], [[65534], [65536]], [[3, 40, 65535], [5, 65536]], [[3, 40, 65534], [5, 65536]], [[100], [101]], [[100], [102]]]
    aimed = [(i, i % 2 == 0) for i in range(6)]
    for gname, fl in (("wma", {"d": (D2, 0)}), ("wmb", {"d": ((500, 484), 0)}), ("wmr", {"r": (R2, 0)}), ("wms", {"r": ((6, 0), 0)})):     # the 4-byte term last / first in the plan
        terms, _ = B.group(gname, 2, docs, fl)
        f = next(iter(fl))
        B.case("width_%s%s_ex" % (gname, f), "PHRASE", terms[f], 0, gname, aimed=aimed)
        B.case("width_%s%s_win" % (gname, f), "PHRASE", terms[f], 4, gname)
        B.case("width_%s%s_near" % (gname, f), "NEAR", terms[f][::-1], 2, gname, perm=[1, 0], aimed=aimed)
    # -- exact: a word below its phrase index, position 0, the rarest term the last word, eight words
    docs = [[[0], [1], [2]], [[0], [1], [3]], [[5], [6, 9], [1, 7]], [[5], [6, 9], [1, 8]], [[4], [0, 5], [1, 6]], [[4], [0, 6], [1, 7]],
            [[9], [1], [0]], [[3, 30], [1, 31], [0, 2, 32]], [[3, 30], [1, 31], [0, 2, 33]]]
    aimed = [(0, True), (1, False), (2, True), (3, False), (4, True), (5, False), (6, False), (7, True), (8, False)]
    terms, _ = B.group("ex3", 3, docs, {"d": ((500, 492, 484), 0), "f": ((500, 492, 0), POS_EDGE_FLAVOUR_STEP)})     # the rarest term is the last word
    for f, names in terms.items():
        B.case("exact_ex3%s" % f, "PHRASE", names, 0, "ex3", aimed=aimed)
    docs, aimed = [], []
    for p_long, n in ((0, 1), (3, 9), (7, 20), (2, 70)):
        for match in (True, False):
            docs.append(_craft_lists("PHRASE", 0, 8, p_long, n, n - 1, match))
            aimed.append((len(docs) - 1, match))
    docs += [[[j] for j in range(8)], [[j if j < 7 else 8] for j in range(8)]]                    # from position 0
    aimed += [(len(docs) - 2, True), (len(docs) - 1, False)]
    terms, _ = B.group("ex8", 8, docs, {"r": (_X8, 0)})
    B.case("exact_ex8r", "PHRASE", terms["r"], 0, "ex8", aimed=aimed)
    # -- window: b - base equal to the window and one more (with every window), a first base that fails and a later one that fits, the greedy
    #    walk's restart from b - window, a later word's list running out
    for T in (2, 3, 4):
        for extra in (1, 3, 40):
            w = T + extra
            docs, aimed = [], []
            for p_long, n in ((0, 1), (T - 1, 9), (0, 20), (T - 1, 70)):
                for match in (True, False):
                    docs.append(_craft_lists("PHRASE", w, T, p_long, n, n // 2, match))
                    aimed.append((len(docs) - 1, match))
            first = [[10 + j, 200 + j] for j in range(T)]
            first[-1] = [10 + w, 200 + w - 1]                                  # base 10 fails by one, base 200 fits at equality
            late = [[10 + j, 300 + j] for j in range(T)]
            late[-1] = [10 + w + 1, 300 + w]                                                          # both bases fail, the second by one
            out = [[10 + j, 400 + j] for j in range(T)]
            out[-1] = [10 + w + 5]                                                                    # the last word's list runs out under the second base
            skip = [[10 + j] for j in range(T)]
            skip[0] = [10, 12 + w, 500]; skip[-1] = [11 + 2 * w]                                      # the restart at b - window passes over a base
            docs += [first, late, out, skip]
            aimed += [(len(docs) - 4, True), (len(docs) - 3, False), (len(docs) - 2, False)]
            fl = {"d": ([480 + 2 * _X8[j] for j in range(T)], 0), "f": ([0 if _X8[j] == min(_X8[:T]) else 480 + 2 * _X8[j] for j in range(T)], POS_EDGE_FLAVOUR_STEP)}
            terms, _ = B.group("v%d%d" % (T, extra), T, docs, fl)
            for f, names in terms.items():
                B.case("window_v%d_%d%s" % (T, extra, f), "PHRASE", names, w, "v%d%d" % (T, extra), aimed=aimed)
    # -- near: span == window - 1 and == window for window n, n + 2, 40 and 70 000; every term order; all heads below the window; the
    #    smallest head's list running out; 2 .. 8 terms
    import itertools
    for T in (2, 3, 4, 6, 8):
        docs, aimed_by = [], {}
        for w in (T, T + 2, 40, 70000):
            for p_long, n in ((0, 1), (T - 1, 9), (T // 2, 20), (0, 70)):
                for match in (True, False):
                    docs.append(_craft_lists("NEAR", w, T, p_long, n, n - 1, match, stride=64 if w < 60 else 80000))
                    aimed_by.setdefault(w, []).append((len(docs) - 1, match))
        low = [[1 + j] for j in range(T)]                                                             # every head below every window
        runs_out = [[5 + j, 5000 + 3 * j] for j in range(T)]
        runs_out[0] = [5]; runs_out[-1] = [4000, 5000 + 3 * T]                                      # term 0 holds the smallest head and has nothing further
        docs += [low, runs_out]
        for w in (T, T + 2, 40, 70000):
            aimed_by[w] += [(len(docs) - 2, True), (len(docs) - 1, w == 70000)]
        # (the lists of the 70 000 window reach past 65 535: these terms have 4-byte lists throughout — the 2-byte NEAR lists are len / idx / plan's)
        terms, _ = B.group("n%d" % T, T, docs, {"r": (_X8[:T], 0)})
        perms = list(itertools.permutations(range(T))) if T <= 3 else [tuple(range(T)), tuple(reversed(range(T))), tuple(rng.sample(range(T), T))]
        for f, names in terms.items():
            for w in (T, T + 2, 40, 70000):
                for pi, perm in enumerate(perms if w in (T, T + 2) else perms[:1]):
                    B.case("near_n%d%s_w%d_o%d" % (T, f, w, pi), "NEAR", [names[j] for j in perm], w, "n%d" % T, perm=perm, aimed=aimed_by[w])
    assert len({c["name"] for c in B.cases}) == len(B.cases)
    live = set(range(1, POS_EDGE_LASTDOCID + 1))
    for d in live:
        if d not in B.doclen:                      # a document no group reached: one filler posting of its own, so that every docid is a document
            B._put("fill", d, [1])
    _pos_edge_cache = B
    return B


def positional_edge_postings():
    """(postings {term: [(did, wdf, [positions])]}, doclen {did: Σ wdf}) of the positional filter's edge corpus: 3 839 documents (15 stripes), built for
    stripe_bits = 8.  Every posting has exactly wdf positions; the positions inside a document are pairwise distinct."""
    B = _positional_edges()
    return B.post, B.doclen


def positional_edge_cases():
    """[dict(name, edge, op, terms, window, first, maxitems, group, perm)]: the table; the name's first word is the edge cell."""
    return [dict(c) for c in _positional_edges().cases]


def positional_edge_lists(case):
    """{docid: the lists in QUERY order} of the case's conjunction (its group), and {docid: intended verdict} for the documents crafted for it."""
    B = _positional_edges()
    lists = {}
    for gname in case["group"] if isinstance(case["group"], list) else [case["group"]]:
        g = B.groups[gname]
        fl = next(f for f, names in g["terms"].items() if set(names) == set(case["terms"]))
        off, perm = g["offs"][fl], case["perm"] or list(range(len(case["terms"])))
        lists.update({d: [[p + off for p in docs[j]] for j in perm] for d, docs in zip(g["dids"], g["docs"])})
    return lists, {d: v for (n, d), v in B.intent.items() if n == case["name"]}


def positional_edge_term_info():
    """{term: dict(dense, wide, extras)}: which terms are meant to have containers, which 4-byte lists."""
    return dict(_positional_edges().term_info)
