#!/usr/bin/env python
"""What lies between two match kernels of consecutive batches in flight, out of ONE rocprofv3 run of the headline loop (CSV, no counters):
  rocprofv3 --kernel-trace --hip-runtime-trace --memory-copy-trace --output-format csv -d DIR -- python bench.py --steps 12 --warmup 3 --no-latency ...

Per pair of consecutive match kernels (i, i + 1) of the timed region:
  (i)   gap_us         idle time of the match stream: start of kernel i + 1 minus end of kernel i
  (ii)  in the window  copies (direction, stream) and other dispatches (fills; kernel name, queue, stream) that overlap (end i, start i + 1)
  (iii) launch_late_us the return of the launch call of kernel i + 1 minus the end of kernel i (<= 0: the launch was queued in time)
  (iv)  end_late_us    per hipEventSynchronize that follows a match kernel's end: its return minus the end of the latest match kernel (and of the
                       latest device-to-host copy) that ended before it — how long xgm_batch_end returns after the batch is complete
and, per batch, the HIP calls that put a packet on a queue (by function) between two launch calls.  Barrier packets themselves (event waits, event
records, the marker of a start event) are not dispatches and do not appear in any of the three traces: what the window holds beyond copies and
fills is inferred from the calls, not seen.

usage: inflight_gap.py <rocprofv3 output dir> [--kernel SUBSTR] [--label NAME] [--out file.json]"""
import argparse
import bisect
import collections
import csv
import glob
import json
import os
import statistics
import sys

PACKET_CALLS = ("hipExtLaunchKernel", "hipLaunchKernel", "hipExtModuleLaunchKernel", "hipModuleLaunchKernel", "hipMemcpyAsync", "hipMemsetAsync", "hipEventRecord",
                "hipStreamWaitEvent", "hipMemcpy", "hipMemset", "hipMemcpyWithStream")


def read(d, suffix):
    files = glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True)
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            rows += list(csv.DictReader(fh))
    return rows


def ts(r, k):
    return int(r[k])


def summary(v):
    v = sorted(v)
    if not v:
        return None
    return {"n": len(v), "median": round(statistics.median(v), 2), "min": round(v[0], 2), "max": round(v[-1], 2),
            "p10": round(v[len(v) // 10], 2), "p90": round(v[(len(v) * 9) // 10], 2)}


def analyse(d, kernel_sub, label):
    kern = read(d, "kernel_trace.csv")
    api = read(d, "hip_api_trace.csv")
    cop = read(d, "memory_copy_trace.csv")
    if not kern:
        sys.exit("no kernel trace under %s" % d)
    if not kernel_sub:                                              # the match kernel: the xgm_ kernel the run spent most time in
        total = collections.Counter()
        for r in kern:
            if "xgm_" in r["Kernel_Name"]:
                total[r["Kernel_Name"]] += ts(r, "End_Timestamp") - ts(r, "Start_Timestamp")
        kernel_sub = total.most_common(1)[0][0]
    match = sorted((r for r in kern if kernel_sub in r["Kernel_Name"]), key=lambda r: ts(r, "Start_Timestamp"))
    other = sorted((r for r in kern if kernel_sub not in r["Kernel_Name"]), key=lambda r: ts(r, "Start_Timestamp"))
    by_corr = {r.get("Correlation_Id"): r for r in api if "Launch" in r.get("Function", "")}
    # the timed region: the longest run of match kernels no further than 1 ms apart (warm-up, timed steps; the legs around it stand apart)
    runs, cur = [], [match[0]]
    for a, b in zip(match, match[1:]):
        if ts(b, "Start_Timestamp") - ts(a, "End_Timestamp") < 1_000_000:
            cur.append(b)
        else:
            runs.append(cur)
            cur = [b]
    runs.append(cur)
    region = max(runs, key=len)
    region = region[len(region) // 4:]                               # (drop the warm-up quarter)
    gaps, late, dur, in_window = [], [], [], collections.Counter()
    windows_with_copy = windows_with_dispatch = 0
    for a, b in zip(region, region[1:]):
        w0, w1 = ts(a, "End_Timestamp"), ts(b, "Start_Timestamp")
        gaps.append((w1 - w0) / 1e3)
        dur.append((ts(a, "End_Timestamp") - ts(a, "Start_Timestamp")) / 1e3)
        lc = by_corr.get(b.get("Correlation_Id"))
        if lc:
            late.append((ts(lc, "End_Timestamp") - w0) / 1e3)
        had_copy = had_disp = False
        for c in cop:
            if ts(c, "Start_Timestamp") < w1 and ts(c, "End_Timestamp") > w0:
                in_window["copy %s stream %s" % (c.get("Direction", "?"), c.get("Stream_Id", "?"))] += 1
                had_copy = True
        for o in other:
            if ts(o, "Start_Timestamp") < w1 and ts(o, "End_Timestamp") > w0:
                in_window["dispatch %s queue %s stream %s" % (o["Kernel_Name"][:40], o.get("Queue_Id", "?"), o.get("Stream_Id", "?"))] += 1
                had_disp = True
        windows_with_copy += had_copy
        windows_with_dispatch += had_disp
    t0, t1 = ts(region[0], "Start_Timestamp"), ts(region[-1], "End_Timestamp")
    # copies anywhere in the region, by direction and stream: where the batches' uploads and downloads run
    copies = collections.Counter("%s stream %s" % (c.get("Direction", "?"), c.get("Stream_Id", "?")) for c in cop if t0 <= ts(c, "Start_Timestamp") <= t1)
    # (iv)
    k_ends = sorted(ts(r, "End_Timestamp") for r in match)
    d2h_ends = sorted(ts(c, "End_Timestamp") for c in cop if "DEVICE_TO_HOST" in c.get("Direction", "").upper().replace(" ", "_"))
    end_late_k, end_late_c, sync_block = [], [], []
    for r in api:
        if r.get("Function") != "hipEventSynchronize" or not (t0 <= ts(r, "End_Timestamp") <= t1 + 2_000_000):
            continue
        e = ts(r, "End_Timestamp")
        i = bisect.bisect_right(k_ends, e)
        if i and k_ends[i - 1] >= ts(r, "Start_Timestamp"):           # (the call waited for that kernel; one that found its event done says nothing)
            end_late_k.append((e - k_ends[i - 1]) / 1e3)
            j = bisect.bisect_right(d2h_ends, e)
            if j and d2h_ends[j - 1] >= k_ends[i - 1]:
                end_late_c.append((e - d2h_ends[j - 1]) / 1e3)
            sync_block.append((e - ts(r, "Start_Timestamp")) / 1e3)
    # packet-producing calls per batch
    launches = sorted((ts(r, "Start_Timestamp") for r in api if "Launch" in r.get("Function", "") and t0 - 500_000 <= ts(r, "Start_Timestamp") <= t1))
    per_batch = collections.Counter()
    if len(launches) > 1:
        for r in api:
            f = r.get("Function", "")
            if f in PACKET_CALLS and launches[0] <= ts(r, "Start_Timestamp") < launches[-1]:
                per_batch[f] += 1
        per_batch = {f: round(n / (len(launches) - 1), 2) for f, n in sorted(per_batch.items())}
    queues = sorted({(r.get("Queue_Id"), r.get("Stream_Id")) for r in region})
    return {"label": label, "kernel": kernel_sub[:60], "pairs": len(gaps), "match_queue_stream": [list(q) for q in queues],
            "kernel_us": summary(dur), "gap_us": summary(gaps), "launch_late_us": summary(late),
            "launch_late_share": round(sum(1 for x in late if x > 0) / len(late), 3) if late else None,
            "windows_with_copy": windows_with_copy, "windows_with_other_dispatch": windows_with_dispatch, "in_window": dict(in_window),
            "copies_in_region": dict(copies), "end_late_after_kernel_us": summary(end_late_k), "end_late_after_d2h_copy_us": summary(end_late_c),
            "event_synchronize_blocked_us": summary(sync_block), "packet_calls_per_batch": per_batch}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--kernel", default="")
    ap.add_argument("--label", default="")
    ap.add_argument("--out")
    a = ap.parse_args()
    res = analyse(a.dir, a.kernel, a.label or os.path.basename(os.path.normpath(a.dir)))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
