#!/usr/bin/env python3
"""Times xgm_filter_build with ONE clause on the synthetic index: a XGM_RANGE_LIST clause on three list columns and the plain
kernel on the ordinals of the first —
  a  every document one element          (xgm_filter_mark_lists_kernel: heads only, ext never read)
  b  10 % of the documents 3 elements    (ascending lists, the rest one element)
  c  every document 3 elements
  d  XGM_RANGE_VALUE on a's ordinals     (xgm_filter_mark_kernel, the kernel every filter ran before list columns)
Lists are attached from memory.  The clause lets about 30 % of the ordinals through.

Per case and repeat: the median over --calls calls (after --warmup) of
  kernel_us   the hipEvent pair xgm_filter_build records around its mark kernel (xgm_index_set_profiling / xgm_last_kernel_ms, read after each
              call); null where the library records none
  wall_us     host clock around the whole call (allocation of the bitmap, launch, the count's copy back, a stream synchronise)
beside
  bound_us    the streaming bound at 8 TB/s: head (or ord) bytes + 32 B x the sectors of ext the walk touches + the padded bitmap's bytes.
The cases are measured --repeats times in turn (a b c d a b c d ...): the spread of d's medians over the repeats is the session's run-to-run
spread, the yardstick for the ratio a / d (a reads the same bytes as d).
--no-events leaves profiling off (kernel_us null): the wall time of the call as a caller sees it.
--plain-only measures d alone and uses nothing a library without list columns lacks: run that way against the parent commit's build, its d is
the yardstick (--parent-json merges its line into this run's output).
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from xapiand_amd import Database, _lib          # noqa: E402

CORPUS_SEED = 0x5EED0001
HBM_BYTES_PER_S = 8e12
N_DISTINCT = 1000
LO, HI = 301, 600


def measure(db, ranges, calls, warmup):
    def once():
        t0 = time.perf_counter()
        flt = db.build_filter(ranges)
        dt = (time.perf_counter() - t0) * 1e6
        ms = db.last_kernel_ms()
        flt.close()
        return dt, ms
    for _ in range(warmup):
        once()
    got = [once() for _ in range(calls)]
    kern = [ms * 1e3 for _, ms in got if ms >= 0]
    return statistics.median(dt for dt, _ in got), (statistics.median(kern) if kern else None)


def ext_sectors(counts, elem, off):
    """32-byte sectors of ext a LIST clause [LO, HI] touches: per multi-element document the words n, first and last, and — unless
    hi < first or lo > last — the elements up to the first one >= lo."""
    multi = np.nonzero(counts >= 2)[0]
    if not len(multi):
        return 0, 0
    n = counts[multi].astype(np.int64)
    base = np.zeros(len(multi), dtype=np.int64)
    base[1:] = np.cumsum(n + 1)[:-1]                                   # ext index of each document's n
    touched = [base, base + 1, base + n]
    first, last = elem[off[multi]], elem[off[multi] + n - 1]
    walk = ~((HI < first) | (LO > last))
    for j in range(1, int(n.max())):                                   # element j + 1 is read when elements 1 .. j were all below lo
        walk = walk & (j < n) & (elem[np.minimum(off[multi] + j - 1, len(elem) - 1)] < LO)
        touched.append((base + 1 + j)[walk])
    words = np.concatenate(touched)
    return int(np.unique(words // 8).size), int((n + 1).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--vocab", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--no-events", action="store_true")
    ap.add_argument("--parent-json")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    emulated = not torch.cuda.is_available()                                   # a rehearsal against tests/emu: its times mean nothing
    if emulated and not __import__("os").environ.get("XGM_LIB_PATH"):
        sys.exit("filter_time.py measures on the GPU: none here")
    db = Database.synthetic(CORPUS_SEED, args.docs, args.vocab, with_positions=False)
    run(db, args, emulated)
    db.close()


def run(db, args, emulated):
    last = db.get_lastdocid()
    rng = np.random.RandomState(1)
    single = rng.randint(1, N_DISTINCT + 1, size=last + 1).astype(np.uint32)
    single[0] = 0
    n_words_padded = (last // 32 + 1 + 63) // 64 * 64
    head_bytes, bitmap_bytes = 4 * (last + 1), 4 * n_words_padded
    u32p = __import__("ctypes").POINTER(__import__("ctypes").c_uint32)
    _lib.check(_lib.lib().xgm_index_attach_column_ordinals(db._h, 200, single.ctypes.data_as(u32p), last + 1, N_DISTINCT))
    inside = lambda x: (x >= LO) & (x <= HI)
    cases = {"d": dict(ranges=[(200, LO, HI)], passing=int(inside(single[1:]).sum()), ext_sectors=0, ext_words=0, kernel="xgm_filter_mark_kernel")}
    if not args.plain_only:
        triple = np.sort(rng.randint(1, N_DISTINCT + 1, size=(last + 1, 3)).astype(np.uint32), axis=1)
        for name, slot, frac in (("a", 201, 0.0), ("b", 202, 0.1), ("c", 203, 1.0)):
            is_multi = (rng.rand(last + 1) < frac) if 0.0 < frac < 1.0 else np.full(last + 1, frac == 1.0)
            is_multi[0] = False
            counts = np.where(is_multi, 3, 1).astype(np.uint32)
            counts[0] = 0
            off = np.zeros(last + 2, dtype=np.uint32)
            off[1:] = np.cumsum(counts, dtype=np.uint64)
            elem = np.zeros(int(off[-1]), dtype=np.uint32)
            s = np.nonzero(~is_multi)[0][1:]                                   # (without docid 0)
            elem[off[s]] = single[s]
            m = np.nonzero(is_multi)[0]
            for j in range(3):
                elem[off[m] + j] = triple[m, j]
            db.attach_list_column_arrays(slot, off, elem, N_DISTINCT)
            ok = np.where(is_multi, inside(triple).any(axis=1), inside(single))      # ascending lists: LIST is "some element inside"
            ok[0] = False
            sectors, words = ext_sectors(counts, elem, off)
            cases[name] = dict(ranges=[(slot, LO, HI, _lib.XGM_RANGE_LIST)], passing=int(ok.sum()), ext_sectors=sectors, ext_words=words,
                               kernel="xgm_filter_mark_lists_kernel")
    for c in cases.values():
        flt = db.build_filter(c["ranges"])
        assert flt.n_docs == c["passing"], (c["ranges"], flt.n_docs, c["passing"])
        flt.close()
        c["bound_us"] = round((head_bytes + 32 * c["ext_sectors"] + bitmap_bytes) / HBM_BYTES_PER_S * 1e6, 2)
        c["kernel_us"], c["wall_us"] = [], []
    if not args.no_events:                                                     # (the event pair costs the call two hipEventRecord: wall times without it are the call's own)
        db.set_profiling(1)
        db.last_kernel_ms()
    for _ in range(args.repeats):
        for name in sorted(cases):
            wall, kern = measure(db, cases[name]["ranges"], args.calls, args.warmup)
            cases[name]["wall_us"].append(round(wall, 2))
            cases[name]["kernel_us"].append(round(kern, 2) if kern is not None else None)
            print(name, cases[name]["wall_us"][-1], cases[name]["kernel_us"][-1], file=sys.stderr, flush=True)
    db.set_profiling(0)
    out = {"tool": "tools/filter_time.py", "emulated": emulated, "docs": last, "calls": args.calls, "warmup": args.warmup, "repeats": args.repeats,
           "events": not args.no_events, "clause": [LO, HI], "n_distinct": N_DISTINCT, "head_bytes": head_bytes, "bitmap_bytes": bitmap_bytes,
           "bound": "(head or ord bytes + 32 B x ext sectors touched + padded bitmap bytes) at 8 TB/s",
           "cases": {k: {f: v for f, v in c.items() if f != "ranges"} for k, c in cases.items()}}
    if args.parent_json:
        with open(args.parent_json) as f:
            out["parent"] = json.loads(f.readline())
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
