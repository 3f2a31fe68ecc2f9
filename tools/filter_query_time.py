#!/usr/bin/env python3
"""Times xgm_filter_build_query and xgm_filter_combine on the synthetic index —
  term_r1, term_r100, term_r10000   a single term of that frequency rank
  and3                              AND of three frequent terms
  or5                               OR of five
  or16                              OR of 16 terms (an accuracy-term set)
  combine                           xgm_filter_combine(AND) of the filters of term_r1 and term_r100
  not, xor                          xgm_filter_combine(XGM_FILTER_NOT) of term_r1's filter; (XGM_FILTER_XOR) of the two: the same three bitmaps as combine
  all                               xgm_filter_all with the index's live set cached: two bitmaps
  all_first                         the ONE xgm_filter_all that makes the live set, on a freshly built (or opened) index: one sample per index,
                                    --first-opens of them, every sample listed; XGM_LIVE_FROM_LENGTHS=1 makes an index without gaps — the synthetic one —
                                    mark its set from the lengths (rule (c): the doclen section in, the bitmap out) instead of by rule (a) (the bitmap out)
  batch10                           ONE xgm_filter_build_query_batch call over ten plans (term_r1, term_r100, term_r10000, and3, or5 and five more of
                                    the same kinds): wall_us / kernel_us of the one call, beside singles_wall_us / singles_kernel_us — the same ten
                                    filters by ten xgm_filter_build_query calls, timed as one sequence (the kernel times summed)
  batch10_under                     the same ten plans under term_r100's filter; the single route is then ten builds and ten xgm_filter_combine(AND)
                                    Against a library from before the batch call (XGM_LIB_PATH) both rows hold the single route alone.
--rows a,b,... measures only those rows (an A/B of one row between two builds of the library).
Per row: the median over --calls calls (after --warmup) of
  kernel_us   the hipEvent pair the call records around its kernel (xgm_index_set_profiling / xgm_last_kernel_ms, read after each call)
  wall_us     host clock around the whole call (allocation of the bitmap, launch, the count's copy back, a stream synchronise)
beside
  bound_us    (1 KB per non-empty (container term, stripe) + 4 B per flat posting read + the padded bitmap's bytes written) at 8 TB/s; for combine
              two bitmaps read and one written, and so for not and xor; for all one read and one written; for all_first the doclen section (rule (c)
              only) and the bitmap written, twice: the set, then the filter's copy.  Which terms have containers is the library's rule (df >= 32 per stripe on average); their non-empty
              stripes and the other terms' postings are counted from the terms' own match lists.
  parent_us   the only route to the same bits without this call: xgm_search_all of the same plan (for combine: of the AND of the two terms) into a
              buffer allocated once, plus setting the bits on the host with numpy; wall clock, median of --parent-calls calls after two.  null where
              xgm_search_all declines the plan (XGM_UNSUPPORTED: the parent has no route to these bits at all) and for all, all_first, not and xor (no
              plan expresses them).
Every row's set bits are checked against the parent route's before anything is timed (where it declines: against the union or intersection of its
answers for the single terms; all, not and xor: against numpy over the single terms' answers and every docid 1 .. lastdocid — the synthetic index has no gaps).  --segment FILE measures an index opened from a segment file instead of the synthetic one (a rehearsal under the kernel
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
# batch10: the first five rows above and five more of the same kinds — a dashboard's ten restrictions, some of whose terms recur
BATCH_ROWS = ROWS[:5] + [("term_r10", "OR", ["t10"]), ("term_r1000", "OR", ["t1000"]), ("term_r50", "OR", ["t50"]), ("and3b", "AND", ["t3", "t11", "t40"]),
                         ("or5b", "OR", ["t12", "t40", "t400", "t3000", "t7"])]


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
    ap.add_argument("--rows", help="comma-separated row names (default: every row)")
    ap.add_argument("--first-opens", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    emulated = not torch.cuda.is_available()                                   # a rehearsal against tests/emu: its times mean nothing
    if emulated and not __import__("os").environ.get("XGM_LIB_PATH"):
        sys.exit("filter_query_time.py measures on the GPU: none here")
    def open_index():
        return Database(args.segment) if args.segment else Database.synthetic(CORPUS_SEED, args.docs, args.vocab, with_positions=False)
    db = open_index()
    names = [n for n, _, _ in ROWS] + ["combine", "not", "xor", "all", "batch10", "batch10_under", "all_first"]
    wanted = set(args.rows.split(",")) if args.rows else set(names)
    assert wanted <= set(names), sorted(wanted - set(names))
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
        if name not in wanted:
            continue
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
    pa, pb = make_plan(db, "OR", ["t1"]), make_plan(db, "OR", ["t100"])
    fa, fb = db.build_query_filter(pa), db.build_query_filter(pb)
    both = make_plan(db, "AND", ["t1", "t100"])
    if "combine" in wanted:
        fc = fa.combine(fb, _lib.XGM_FILTER_AND)
        assert (np.array(fc.words(), dtype=np.uint32) == parent.words(both)).all()
        rows["combine"] = dict(terms=["t1", "t100"], op="filter AND filter", n_docs=fc.n_docs, kernel="xgm_filter_combine_kernel", has_parent=True,
                               bound_us=round(3 * bitmap_bytes / HBM_BYTES_PER_S * 1e6, 3), build=(lambda: fa.combine(fb, _lib.XGM_FILTER_AND)), parent_plan=both)
        fc.close()
    # the rows without a parent route: numpy over the single terms' answers and the live set, which on an index without gaps is every docid 1 .. lastdocid
    live = np.zeros((last + 32) // 32 * 32, dtype=np.uint8)
    live[1:last + 1] = 1
    live = np.packbits(live, bitorder="little").view("<u4")
    if wanted & {"not", "xor", "all", "all_first"}:
        assert args.segment or db.get_doccount() == last
        wa, wb = parent.words(pa), parent.words(pb)
        new = {"not": ("NOT filter", ["t1"], 3, lambda: fa.combine(None, _lib.XGM_FILTER_NOT), live & ~wa),
               "xor": ("filter XOR filter", ["t1", "t100"], 3, lambda: fa.combine(fb, _lib.XGM_FILTER_XOR), wa ^ wb),
               "all": ("MatchAll, the live set cached", [], 2, lambda: db.filter_all(), live)}
        for name, (op, terms, n_maps, build, want) in new.items():
            if name not in wanted:
                continue
            flt = build()
            assert (np.array(flt.words(), dtype=np.uint32) == want).all() and flt.n_docs == int(np.unpackbits(want.view(np.uint8)).sum()), name
            print("checked", name, flt.n_docs, "numpy", file=sys.stderr, flush=True)
            rows[name] = dict(terms=terms, op=op, n_docs=flt.n_docs, kernel="xgm_filter_combine_kernel", has_parent=False,
                              bound_us=round(n_maps * bitmap_bytes / HBM_BYTES_PER_S * 1e6, 3), build=build, parent_plan=None)
            flt.close()
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
    # ten plans at once: ONE xgm_filter_build_query_batch call beside the same ten filters by ten single calls (+ ten combines)
    for name in ("batch10", "batch10_under"):
        if name not in wanted:
            continue
        plans10 = [make_plan(db, op, terms) for _, op, terms in BATCH_ROWS]
        under = fb if name == "batch10_under" else None

        def singles():
            """The single-call route: (the ten filters, the sum of the calls' kernel times in µs or None)."""
            out, kern = [], 0.0
            for p in plans10:
                f = db.build_query_filter(p)
                ms = [db.last_kernel_ms()]
                if under is not None:
                    one, f = f, f.combine(under, _lib.XGM_FILTER_AND)
                    ms.append(db.last_kernel_ms())
                    one.close()
                out.append(f)
                kern = None if kern is None or min(ms) < 0 else kern + sum(ms) * 1e3
            return out, kern

        def batch():
            out = db.build_query_filters(plans10, under)
            ms = db.last_kernel_ms()
            return out, (ms * 1e3 if ms >= 0 else None)
        has_batch = hasattr(db, "build_query_filters")                           # (an A/B against a library from before the call: the single route alone)
        ref, _ = singles()
        r = dict(plans=[n for n, _, _ in BATCH_ROWS], under="term_r100" if under is not None else None, n_docs=[f.n_docs for f in ref],
                 kernel="xgm_filter_mark_query_batch_kernel", launches_single=len(ref) * (2 if under is not None else 1))
        if has_batch:
            got, _ = batch()
            for g, f in zip(got, ref):
                assert g.words() == f.words() and g.n_docs == f.n_docs, name
            info = (C.c_uint64 * 4)()
            _lib.lib().xgm_debug_filter_batch_info(info)
            r.update(launches=int(info[0]), work_items=int(info[1]), waves=int(info[2]), skipped_items=int(info[3]))
            for g in got:
                g.close()
            print("checked", name, r["n_docs"], "the single-call route", file=sys.stderr, flush=True)
        for f in ref:
            f.close()
        db.set_profiling(1)
        db.last_kernel_ms()
        for key, fn in (("batch", batch if has_batch else None), ("singles", singles)):
            if fn is None:
                r["wall_us"] = r["kernel_us"] = None
                continue
            got = []
            for i in range(args.warmup + args.calls):
                t0 = time.perf_counter()
                fs, kern = fn()
                dt = (time.perf_counter() - t0) * 1e6
                for f in fs:
                    f.close()
                if i >= args.warmup:
                    got.append((dt, kern))
            kerns = [k for _, k in got if k is not None]
            wall, kern = round(statistics.median(dt for dt, _ in got), 2), (round(statistics.median(kerns), 2) if kerns else None)
            if key == "batch":
                assert db.last_kernel_name() == r["kernel"], (name, db.last_kernel_name())
                r["wall_us"], r["kernel_us"] = wall, kern
            else:
                r["singles_wall_us"], r["singles_kernel_us"] = wall, kern
        db.set_profiling(0)
        r["wall_ratio"] = round(r["singles_wall_us"] / r["wall_us"], 2) if r["wall_us"] else None
        rows[name] = dict(r, bound_us=None, parent_us=None, below_parent=None)
        print(name, r["kernel_us"], r["wall_us"], "singles", r["singles_kernel_us"], r["singles_wall_us"], file=sys.stderr, flush=True)
    db.set_profiling(0)
    for f in (fa, fb):
        f.close()
    if "all_first" in wanted:
        # one sample per index: the call that makes the live set (the marking kernel, its count's copy back) and the filter's copy of it
        samples, source = [], None
        for i in range(args.first_opens):
            d2 = open_index()
            d2.set_profiling(1)
            d2.last_kernel_ms()
            t0 = time.perf_counter()
            flt = d2.filter_all()
            wall = (time.perf_counter() - t0) * 1e6
            ms = d2.last_kernel_ms()
            info = (C.c_uint64 * 4)()
            _lib.check(_lib.lib().xgm_debug_live_info(d2._h, info))
            assert info[0] == 1 and info[2] == 1
            source = {1: "no gaps: rule (a), the lengths are not read", 3: "the lengths: rule (c)"}[info[1]]
            if i == 0:
                assert (np.array(flt.words(), dtype=np.uint32) == live).all() and flt.n_docs == d2.get_doccount()
            samples.append(dict(wall_us=round(wall, 2), kernel_us=round(ms * 1e3, 2) if ms >= 0 else None))
            flt.close()
            d2.close()
        in_bytes = 4 * (last + 1) if info[1] == 3 else 0
        rows["all_first"] = dict(op="MatchAll, the call that makes the live set", source=source, samples=samples,
                                 wall_us=statistics.median(x["wall_us"] for x in samples),
                                 kernel_us=statistics.median(x["kernel_us"] for x in samples) if all(x["kernel_us"] is not None for x in samples) else None,
                                 bound_us=round((in_bytes + bitmap_bytes + 2 * bitmap_bytes) / HBM_BYTES_PER_S * 1e6, 3), parent_us=None, below_parent=None,
                                 note="kernel_us: the event pair spans the marking kernel, the host's wait for its count and the copying kernel")
        print("all_first", rows["all_first"]["kernel_us"], rows["all_first"]["wall_us"], rows["all_first"]["bound_us"], source, file=sys.stderr, flush=True)
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
