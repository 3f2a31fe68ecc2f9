#!/usr/bin/env python3
"""Times xgm_filter_count_pairs on the synthetic index: three filters (about 1 %, 30 % and 100 % of the documents), three pairs of
slots — 9 x 9 values (counters in LDS), 9 x 1000 (counters by global atomics), 1000 x every-document-distinct (the table).

Per case: the median over the calls (after --warmup) of ONE call with room for every pair (the room is asked for once, before)
  kernel_us   hipEvent pair around the call's kernels (xgm_index_set_profiling / xgm_last_kernel_ms: one pair per call, read after each call)
  wall_us     host clock around the whole call: launches, the copy back of the records and, for the table, the host's sort
  sort_share  the host sort's part of wall_us (xgm_debug_pairs_info; the table only)
beside
  bound_us    the streaming bound at 8 TB/s: bitmap bytes + 32 B x the sectors that hold a passing document (a sector = 8 ordinals) per column read
              + the counters' (4 B x P) or the table's (12 B x S) bytes
  parent_*    the parent commit's nearest thing: xgm_search_range under docid order with the one-slot spy on the FIRST of the two slots, same filter.
              It reads one column and cannot answer the question.  Informational.
--calls is what a case runs when a call takes under --budget-s / --calls seconds; a slower case (the table at 10 M pairs: a 160 MB copy back and a
sort of 10 M records per call) runs as many calls as fit --budget-s, at least 5, and says so ("calls").
Prints one JSON line (and writes it to --out)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xapiand_amd import Database, _lib          # noqa: E402
from xapiand_amd.enquire import search_range          # noqa: E402

CORPUS_SEED = 0x5EED0001
HBM_BYTES_PER_S = 8e12


def attach(db, slot, ords, n_distinct):
    o = np.ascontiguousarray(ords, dtype=np.uint32)
    _lib.check(_lib.lib().xgm_index_attach_column_ordinals(db._h, slot, o.ctypes.data_as(C.POINTER(C.c_uint32)), len(o), n_distinct))


def timed(f, calls, warmup, after):
    for _ in range(warmup):
        f()
        after()
    wall, extra = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        f()
        wall.append((time.perf_counter() - t0) * 1e6)
        extra.append(after())
    return wall, extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--vocab", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--budget-s", type=float, default=15.0)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    emulated = bool(os.environ.get("XGM_LIB_PATH"))              # a rehearsal of the script against tests/emu: its times mean nothing
    if not torch.cuda.is_available() and not emulated:
        sys.exit("pairs_time.py measures on the GPU: none here")
    l = _lib.lib()
    db = Database.synthetic(CORPUS_SEED, args.docs, args.vocab, with_positions=False)
    last = db.get_lastdocid()
    rng = np.random.RandomState(1)
    cols = {100: rng.randint(1, 10, size=last + 1).astype(np.uint32), 102: rng.randint(1, 10, size=last + 1).astype(np.uint32),
            103: rng.randint(1, 1001, size=last + 1).astype(np.uint32), 101: np.zeros(last + 1, dtype=np.uint32)}
    cols[101][1:] = rng.permutation(last) + 1
    nd = {100: 9, 102: 9, 103: 1000, 101: last}
    for slot in cols:
        attach(db, slot, cols[slot], nd[slot])
    filters = {"1%": [(101, 1, max(1, last // 100))], "30%": [(101, 1, max(1, 3 * last // 10))], "100%": [(100, 1, _lib.XGM_ORD_MAX)]}
    slot_pairs = {"9x9": (100, 102), "9x1000": (100, 103), "1000xdistinct": (103, 101)}
    n_words_padded = (last // 32 + 1 + 63) // 64 * 64
    info = (C.c_uint64 * 4)()
    cases = []
    for fname, ranges in filters.items():
        ok = np.ones(last + 1, dtype=bool)
        for slot, lo, hi in ranges:
            ok &= (cols[slot] >= lo) & (cols[slot] <= hi) & (cols[slot] != 0)
        ok[0] = False
        sectors = int(np.unique(np.nonzero(ok)[0] // 8).size)
        flt = db.build_filter(ranges)
        assert flt.n_docs == int(ok.sum())
        for pname, (sa, sb) in slot_pairs.items():
            n = C.c_uint64()
            _lib.check(l.xgm_filter_count_pairs(db._h, flt._h, sa, sb, None, 0, C.byref(n)))
            room = n.value
            buf = np.zeros((max(room, 1), 4), dtype=np.uint32)
            pbuf = buf.ctypes.data_as(C.POINTER(_lib.PairCount))
            call = lambda: _lib.check(l.xgm_filter_count_pairs(db._h, flt._h, sa, sb, pbuf, room, C.byref(n)))
            sort_ns = []

            def after():
                l.xgm_debug_pairs_info(info)
                sort_ns.append(info[3])
                return db.last_kernel_ms()
            db.set_profiling(1)
            db.last_kernel_ms()
            t0 = time.perf_counter()
            call()
            after()
            once = time.perf_counter() - t0
            calls = args.calls if once * args.calls <= args.budget_s else max(5, int(args.budget_s / once))
            warmup = args.warmup if calls == args.calls else 2
            del sort_ns[:]
            wall, kern_ms = timed(call, calls, warmup, after)
            db.set_profiling(0)
            assert n.value == room and int(buf[:room, 2].sum()) == flt.n_docs
            l.xgm_debug_pairs_info(info)
            path, slots = int(info[0]), int(info[1])
            table_bytes = slots * (12 if path == 3 else 4)
            bound_us = (n_words_padded * 4 + 32 * sectors * 2 + table_bytes) / HBM_BYTES_PER_S * 1e6
            wall_us = statistics.median(wall)
            sort_us = statistics.median(sort_ns[-calls:]) / 1e3
            db.set_profiling(1)
            db.last_kernel_ms()
            pwall, pkern = timed(lambda: search_range(db, flt, 10, spy=(sa, nd[sa])), max(5, min(calls, 50)), 3, db.last_kernel_ms)
            db.set_profiling(0)
            cases.append({"filter": fname, "passing": flt.n_docs, "slots": pname, "path": {1: "dense, LDS", 2: "dense, global", 3: "sparse"}[path],
                          "counters_or_slots": slots, "n_pairs": room, "calls": calls, "kernel_us": round(statistics.median(kern_ms) * 1e3, 2),
                          "wall_us": round(wall_us, 2), "sort_share": round(sort_us / wall_us, 3) if path == 3 else None, "bound_us": round(bound_us, 2),
                          "parent_kernel_us": round(statistics.median(pkern) * 1e3, 2), "parent_wall_us": round(statistics.median(pwall), 2)})
            print(cases[-1], file=sys.stderr, flush=True)
        flt.close()
    line = json.dumps({"tool": "tools/pairs_time.py", "emulated": emulated, "docs": last, "calls": args.calls, "warmup": args.warmup,
                       "bound": "(bitmap bytes + 32 B x sectors holding a passing document x 2 columns + 4 B x counters or 12 B x table slots) at 8 TB/s",
                       "parent": "xgm_search_range, docid order, k = 10, one-slot spy on the first of the two slots, same filter", "cases": cases})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    db.close()


if __name__ == "__main__":
    main()
