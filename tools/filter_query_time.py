#!/usr/bin/env python3
"""Times xgm_filter_build_query and xgm_filter_combine on the synthetic index —
  term_r1, term_r100, term_r10000   a single term of that frequency rank
  and3                              AND of three frequent terms
  or5                               OR of five
  or16                              OR of 16 terms (an accuracy-term set)
  combine                           xgm_filter_combine(AND) of the filters of term_r1 and term_r100
Per row: the median over --calls calls (after --warmup) of
  kernel_us   the hipEvent pair the call records around its kernel (xgm_index_set_profiling / xgm_last_kernel_ms, read after each call)
  wall_us     host clock around the whole call (allocation of the bitmap, launch, the count's copy back, a stream synchronise)
beside
  bound_us    (1 KB per non-empty (container term, stripe) + 4 B per flat posting read + the padded bitmap's bytes written) at 8 TB/s; for combine
              two bitmaps read and one written.  Which terms have containers is the library's rule (df >= 32 per stripe on average); their non-empty
              stripes and the other terms' postings are counted from the terms' own match lists.
  parent_us   the only route to the same bits without this call: xgm_search_all of the same plan (for combine: of the AND of the two terms) into a
              buffer allocated once, plus setting the bits on the host with numpy; wall clock, median of --parent-calls calls after two.  null where
              xgm_search_all declines the plan (XGM_UNSUPPORTED: the parent has no route to these bits at all).
Every row's set bits are checked against the parent route's before anything is timed (where it declines: against the union or intersection of its
answers for the single terms).  --segment FILE measures an index opened from a segment file instead of the synthetic one (a rehearsal under the kernel
emulation: its times mean nothing).
Prints one JSON line (and writes it to --out)."""
import argparse
import ctypes as C
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from xapiand_amd import Database, Query, _lib          # noqa: E402
from xapiand_amd.enquire import plan                   # noqa: E402

CORPUS_SEED = 0x5EED0001
HBM_BYTES_PER_S = 8e12
ROWS = [("term_r1", "OR", ["t1"]), ("term_r100", "OR", ["t100"]), ("term_r10000", "OR", ["t10000"]), ("and3", "AND", ["t3", "t7", "t15"]),
        ("or5", "OR", ["t9", "t40", "t300", "t2000", "t7"]), ("or16", "OR", ["t%d" % (200 + 37 * i) for i in range(16)])]


def make_plan(db, op, terms):
    return plan(db, Query(terms[0]) if len(terms) == 1 else Query(op, terms), 0, 10)


class Parent:
    """xgm_search_all + the bits on the host."""

    def __init__(self, db):
        self.db, self.last = db, db.get_lastdocid()
        self.hits, self.cap = None, 0

    def docids(self, p):
        cap = max(1, p.est_max or self.db.get_doccount())
        if cap > self.cap:
            self.hits, self.cap = (_lib.Hit * cap)(), cap
        n, hdr = C.c_uint64(), _lib.ResultHdr()
        _lib.check(_lib.lib().xgm_search_all(self.db._h, C.byref(p), self.hits, self.cap, C.byref(n), C.byref(hdr)))
        assert n.value <= self.cap
        return np.frombuffer(self.hits, dtype=np.uint32, count=4 * n.value).reshape(-1, 4)[:, 0] if n.value else np.zeros(0, dtype=np.uint32)

    def words(self, p):
        ok = np.zeros((self.last + 32) // 32 * 32, dtype=np.uint8)
        ok[self.docids(p)] = 1
        return np.packbits(ok, bitorder="little").view("<u4")

    def supports(self, p):
        try:
            self.docids(p)
            return True
        except _lib.XgmUnsupported:
            return False

    def time(self, p, calls):
        for _ in range(2):
            self.words(p)
        ts = []
        for _ in range(calls):
            t0 = time.perf_counter()
            self.words(p)
            ts.append((time.perf_counter() - t0) * 1e6)
        return statistics.median(ts)


def measure(db, build, calls, warmup):
    def once():
        t0 = time.perf_counter()
        flt = build()
        dt = (time.perf_counter() - t0) * 1e6
        ms = db.last_kernel_ms()
        flt.close()
        return dt, ms
    for _ in range(warmup):
        once()
    got = [once() for _ in range(calls)]
    kern = [ms * 1e3 for _, ms in got if ms >= 0]
    return statistics.median(dt for dt, _ in got), (statistics.median(kern) if kern else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--vocab", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parent-calls", type=int, default=20)
    ap.add_argument("--segment")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    emulated = not torch.cuda.is_available()                                   # a rehearsal against tests/emu: its times mean nothing
    if emulated and not __import__("os").environ.get("XGM_LIB_PATH"):
        sys.exit("filter_query_time.py measures on the GPU: none here")
    db = Database(args.segment) if args.segment else Database.synthetic(CORPUS_SEED, args.docs, args.vocab, with_positions=False)
    last = db.get_lastdocid()
    n_stripes = (last >> 13) + 1
    n_words = (last + 32) // 32
    bitmap_bytes = 4 * ((n_words + 63) // 64 * 64)
    parent = Parent(db)
    per_term = {}                                                              # term -> (container?, non-empty stripes, postings)

    def term_bytes(t):
        if t not in per_term:
            p1 = make_plan(db, "OR", [t])
            d = parent.docids(p1)
            per_term[t] = (len(d) >= 32 * n_stripes, int(np.unique(d >> 13).size), len(d), parent.words(p1))
        dense, stripes, df, _ = per_term[t]
        return 1024 * stripes if dense else 4 * df
    rows = {}
    for name, op, terms in ROWS:
        p = make_plan(db, op, terms)
        bound = round((sum(term_bytes(t) for t in terms) + bitmap_bytes) / HBM_BYTES_PER_S * 1e6, 3)
        has_parent = parent.supports(p)
        want = parent.words(p) if has_parent else (np.bitwise_or if op == "OR" else np.bitwise_and).reduce([per_term[t][3] for t in terms])
        flt = db.build_query_filter(p)
        assert (np.array(flt.words(), dtype=np.uint32) == want).all(), name
        print("checked", name, flt.n_docs, "parent route" if has_parent else "parent declines", file=sys.stderr, flush=True)
        rows[name] = dict(terms=terms, op=op, n_docs=flt.n_docs, containers=0, kernel="xgm_filter_mark_query_kernel", bound_us=bound, has_parent=has_parent)
        rows[name]["containers"] = sum(1 for t in terms if per_term[t][0])
        flt.close()
        rows[name]["build"] = (lambda p=p: db.build_query_filter(p))
        rows[name]["parent_plan"] = p
    fa, fb = db.build_query_filter(rows["term_r1"]["parent_plan"]), db.build_query_filter(rows["term_r100"]["parent_plan"])
    both = make_plan(db, "AND", ["t1", "t100"])
    fc = fa.combine(fb, _lib.XGM_FILTER_AND)
    assert (np.array(fc.words(), dtype=np.uint32) == parent.words(both)).all()
    rows["combine"] = dict(terms=["t1", "t100"], op="filter AND filter", n_docs=fc.n_docs, kernel="xgm_filter_combine_kernel", has_parent=True,
                           bound_us=round(3 * bitmap_bytes / HBM_BYTES_PER_S * 1e6, 3), build=(lambda: fa.combine(fb, _lib.XGM_FILTER_AND)), parent_plan=both)
    fc.close()
    db.set_profiling(1)
    db.last_kernel_ms()
    for name, r in rows.items():
        wall, kern = measure(db, r.pop("build"), args.calls, args.warmup)
        assert db.last_kernel_name() == r["kernel"], (name, db.last_kernel_name())
        r["wall_us"], r["kernel_us"] = round(wall, 2), (round(kern, 2) if kern is not None else None)
        db.set_profiling(0)
        pp = r.pop("parent_plan")
        r["parent_us"] = round(parent.time(pp, args.parent_calls), 2) if r.pop("has_parent") else None
        db.set_profiling(1)
        r["below_parent"] = None if r["parent_us"] is None else r["wall_us"] < r["parent_us"]
        print(name, r["kernel_us"], r["wall_us"], r["bound_us"], r["parent_us"], file=sys.stderr, flush=True)
    db.set_profiling(0)
    for f in (fa, fb):
        f.close()
    out = {"tool": "tools/filter_query_time.py", "emulated": emulated, "docs": last, "stripes": n_stripes, "calls": args.calls, "warmup": args.warmup,
           "parent_calls": args.parent_calls, "bitmap_bytes": bitmap_bytes,
           "bound": "(1 KB per non-empty (container term, stripe) + 4 B per flat posting + padded bitmap bytes) at 8 TB/s; combine: three bitmaps",
           "parent": "xgm_search_all of the same plan + the bits set on the host (numpy), wall clock", "rows": rows,
           "all_below_parent": all(r["below_parent"] is not False for r in rows.values())}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    db.close()


if __name__ == "__main__":
    main()
