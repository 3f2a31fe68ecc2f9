#!/usr/bin/env python3
"""Times xgm_search_range on the synthetic index: three filters (about 1 %, 30 % and 100 % of the documents), three orderings
(docid, a 9-value sort column, an every-document-distinct sort column), each with and without a spy on the 9-value column.

Per case: the median over --calls calls (after --warmup) of
  kernel_us   hipEvent pair around the call's kernels (xgm_index_set_profiling / xgm_last_kernel_ms: one pair per call, read after each call)
  wall_us     host clock around the whole call (it ends in a stream synchronise)
beside
  bound_us    the streaming bound of its passes at 8 TB/s: every digit pass (and a spy-only pass under docid order) and the count pass read the
              bitmap once plus, per column they read, the 32-byte sectors that hold a passing document (a sector = 8 ordinals):
              sum over passes of (bitmap bytes + 32 B x sectors per column read) / 8e12.  The place pass touches only the tiles of the page
              and the finish kernel 1024 pairs: neither is counted.
  parent_wall_us   the only way the parent commit gives the same page: xgm_search_filtered under XGM_SORT_VALUE with the index's most frequent
              term as the query on the same filter (value orders only; it matches fewer documents, which flatters it).  Informational.
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
from xapiand_amd.enquire import plan, search_filtered, search_range          # noqa: E402

CORPUS_SEED = 0x5EED0001
HBM_BYTES_PER_S = 8e12


def attach(db, slot, ords, n_distinct):
    o = np.ascontiguousarray(ords, dtype=np.uint32)
    _lib.check(_lib.lib().xgm_index_attach_column_ordinals(db._h, slot, o.ctypes.data_as(C.POINTER(C.c_uint32)), len(o), n_distinct))


def median_us(f, calls, warmup, after=None):
    for _ in range(warmup):
        f()
        if after:
            after()
    wall, extra = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        f()
        wall.append((time.perf_counter() - t0) * 1e6)
        if after:
            extra.append(after())
    return statistics.median(wall), (statistics.median(extra) if extra else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--vocab", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    emulated = bool(__import__("os").environ.get("XGM_LIB_PATH"))              # a rehearsal of the script against tests/emu: its times mean nothing
    if not torch.cuda.is_available() and not emulated:
        sys.exit("range_time.py measures on the GPU: none here")
    db = Database.synthetic(CORPUS_SEED, args.docs, args.vocab, with_positions=False)
    last = db.get_lastdocid()
    rng = np.random.RandomState(1)
    nine = rng.randint(1, 10, size=last + 1).astype(np.uint32)                    # slot 100: 9 values, every document has one
    distinct = np.zeros(last + 1, dtype=np.uint32)                                # slot 101: every document its own ordinal
    distinct[1:] = rng.permutation(last) + 1
    attach(db, 100, nine, 9)
    attach(db, 101, distinct, last)
    cols = {100: nine, 101: distinct}
    filters = {"1%": [(101, 1, max(1, last // 100))], "30%": [(101, 1, max(1, 3 * last // 10))], "100%": [(100, 1, _lib.XGM_ORD_MAX)]}
    orders = {"docid": None, "nine": 100, "distinct": 101}
    top = plan(db, Query("OR", ["t1"]), 0, args.k)                                # the most frequent term of the synthetic corpus
    n_words_padded = (last // 32 + 1 + 63) // 64 * 64
    cases = []
    for fname, ranges in filters.items():
        ok = np.ones(last + 1, dtype=bool)
        for slot, lo, hi in ranges:
            ok &= (cols[slot] >= lo) & (cols[slot] <= hi) & (cols[slot] != 0)
        ok[0] = False
        sectors = int(np.unique(np.nonzero(ok)[0] // 8).size)
        flt = db.build_filter(ranges)
        assert flt.n_docs == int(ok.sum())
        for oname, slot in orders.items():
            for spy in (None, (100, 9)):
                n_distinct = {None: 0, 100: 9, 101: last}[slot]
                digit_passes = 0 if slot is None else (max(1, n_distinct.bit_length()) + 10) // 11
                # (passes, columns read in each): the digit passes, the first one with the spy column unless it is the sort column; the count pass
                col_reads = [1] * digit_passes
                if spy and slot is not None and slot != spy[0]:
                    col_reads[0] += 1
                if spy and slot is None:
                    col_reads.append(1)                                           # the spy's own pass
                col_reads.append(0 if slot is None else 1)                        # count
                bound_us = sum(n_words_padded * 4 + 32 * sectors * c for c in col_reads) / HBM_BYTES_PER_S * 1e6
                mode = _lib.XGM_SORT_VALUE if slot is not None else None
                db.set_profiling(1)
                db.last_kernel_ms()
                wall, kern_ms = median_us(lambda: search_range(db, flt, args.k, mode, slot or 0, False, spy=spy), args.calls, args.warmup, db.last_kernel_ms)
                db.set_profiling(0)
                parent = None
                if slot is not None:
                    parent, _ = median_us(lambda: search_filtered(db, top, flt, _lib.XGM_SORT_VALUE, slot, False, spy=spy), max(5, args.calls // 10), 2)
                cases.append({"filter": fname, "passing": flt.n_docs, "order": oname, "spy": bool(spy), "digit_passes": digit_passes,
                              "kernel_us": round(kern_ms * 1e3, 2), "wall_us": round(wall, 2), "bound_us": round(bound_us, 2),
                              "parent_wall_us": round(parent, 2) if parent is not None else None})
                print(cases[-1], file=sys.stderr, flush=True)
        flt.close()
    line = json.dumps({"tool": "tools/range_time.py", "emulated": emulated, "docs": last, "k": args.k, "calls": args.calls, "warmup": args.warmup,
                       "bound": "sum over digit/spy/count passes of (bitmap bytes + 32 B x sectors holding a passing document per column read) at 8 TB/s",
                       "parent": "xgm_search_filtered, XGM_SORT_VALUE, query = the most frequent term, same filter (wall clock)", "cases": cases})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    db.close()


if __name__ == "__main__":
    main()
