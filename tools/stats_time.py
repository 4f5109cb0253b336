#!/usr/bin/env python3
"""Timing of the matrix-free similarity statistics on one MI355X.

    python tools/stats_time.py [--n 50000] [--n-dense 20000] [--reps 3] [--out FILE]      the timings
    python tools/stats_time.py --kernels-only [--n 50000]                                 one warm-up + one traced call of (a), for a kernel trace
        (rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/stats_time.py --kernels-only)
    python tools/stats_time.py --summarise-trace DIR [--call-ms MS]                        per-kernel totals of that trace and their share of a call

k = 4, n_hash = 50.  Input: synth.h3n2_like(n, 20).  Host clock around calls that end in a device synchronise, 1 warm-up call, --reps timed
calls per leg, legs alternated in one process; every leg is reported as min / median / max.

  a  similarityMH_stats(seqs) at the host boundary: upload, signatures, planes, compare, histogram, extrema, 20 bytes a row to the host
  b  the yardstick it sits beside: similarityMH_edges(seqs, thresh_p=0.8) on the same input -- the same compare and histogram, then the edges
  c  the dense way, at --n-dense: similarityMH (the float64 matrix to the host) + compute_similarity_stats on it; (a) at that n beside it
  d  (from the kernel trace) k_upper_extrema against k_upper_histogram on the same matrix
"""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, N_HASH, SEED, P = 4, 50, 12345, 0.8


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"min": float(a[0]), "median": float(np.median(a)), "max": float(a[-1]), "reps": len(a)}


def fmt(s):
    return "min %10.3f  median %10.3f  max %10.3f ms  (%d reps)" % (s["min"], s["median"], s["max"], s["reps"])


def summarise(trace_dir, call_ms, say):
    """kernel totals of the LAST traced call (the trace holds a warm-up call and the traced one, each ending with k_upper_extrema)"""
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % trace_dir)
    rows = []
    for f in files:
        for r in csv.DictReader(open(f)):
            k = {key.lower(): v for key, v in r.items()}
            rows.append((int(k["start_timestamp"]), int(k["end_timestamp"]), k["kernel_name"]))
    rows.sort()
    ends = [t for t, (_, _, name) in enumerate(rows) if "k_upper_extrema" in name]
    rows = rows[ends[-2] + 1:] if len(ends) >= 2 else rows
    total = {}
    for b, e, name in rows:
        short = name.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").replace("da::", "")
        c, ms = total.get(short, (0, 0.0))
        total[short] = (c + 1, ms + (e - b) * 1e-6)
    all_ms = sum(ms for _, ms in total.values())
    say("kernels of one similarityMH_stats call (rocprofv3 --kernel-trace, a run of its own), device time %.3f ms%s"
        % (all_ms, "" if call_ms is None else "; share of the call's %.1f ms at the host boundary" % call_ms))
    say("%-44s %6s %12s %9s" % ("kernel", "calls", "ms", "share"))
    for name, (c, ms) in sorted(total.items(), key=lambda kv: -kv[1][1]):
        say("%-44s %6d %12.3f %8.3f%%" % (name[:44], c, ms, 100 * ms / (call_ms if call_ms else all_ms)))
    ex = sum(ms for name, (_, ms) in total.items() if "k_upper_extrema" in name)
    hi = sum(ms for name, (_, ms) in total.items() if "k_upper_histogram" in name)
    say("(d) k_upper_extrema %.3f ms against k_upper_histogram %.3f ms: %.2f x; the pair %.3f ms = %.2f %% of %s"
        % (ex, hi, ex / hi if hi else float("nan"), ex + hi, 100 * (ex + hi) / (call_ms if call_ms else all_ms), "the call" if call_ms else "the device time"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--n-dense", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--summarise-trace", default=None)
    ap.add_argument("--call-ms", type=float, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def finish():
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
    if a.summarise_trace:
        summarise(a.summarise_trace, a.call_ms, say)
        return finish()
    import torch
    import dynaalign_amd as da
    from dynaalign_amd import _capi, synth
    if _capi.load().da_device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured")
    seqs = synth.to_strings(*synth.h3n2_like(a.n, 20))
    stats_call = lambda: da.similarityMH_stats(seqs, K, N_HASH, seed=SEED)   # noqa: E731
    if a.kernels_only:
        stats_call()
        stats_call()
        torch.cuda.synchronize()
        return
    small = seqs[:a.n_dense]
    legs = {"a  similarityMH_stats, n = %d" % a.n: stats_call,
            "b  similarityMH_edges, n = %d" % a.n: lambda: da.similarityMH_edges(seqs, K, N_HASH, P, seed=SEED)[0],
            "c  similarityMH + compute_similarity_stats, n = %d" % a.n_dense:
                lambda: da.compute_similarity_stats(da.similarityMH(small, K, N_HASH, seed=SEED)),
            "a' similarityMH_stats, n = %d" % a.n_dense: lambda: da.similarityMH_stats(small, K, N_HASH, seed=SEED)}
    out = {k: [] for k in legs}
    keep = {}
    for r in range(1 + a.reps):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            keep[name] = fn()
            torch.cuda.synchronize()
            if r >= 1:
                out[name].append((time.perf_counter() - t) * 1e3)
    r = {k: stats(v) for k, v in out.items()}
    names = list(legs)
    dense, free = keep[names[2]], keep[names[3]]
    assert tuple(dense[1:]) == tuple(free[1:]) and abs(dense[0] - free[0]) <= 2.0 ** -40 * dense[0], (dense, free)
    say("similarity statistics without the matrix on the host, k = %d, n_hash = %d; 1 warm-up + %d timed calls per leg, legs alternated" % (K, N_HASH, a.reps))
    say("input: synth.h3n2_like(%d, 20): %d pairs; %r" % (a.n, a.n * (a.n - 1) // 2, keep[names[0]]))
    say("(c) and (a') agree: the doubles bit for bit but the mean (2 ** -40 relative), the positions as integers")
    for k_, v in r.items():
        say("  %-52s %s" % (k_, fmt(v)))
    am, bm, cm, a2m = (r[k_]["median"] for k_ in names)
    say("  a / b = %.2f;  c / a' = %.2f at n = %d" % (am / bm, cm / a2m, a.n_dense))
    finish()


if __name__ == "__main__":
    main()
