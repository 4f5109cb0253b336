#!/usr/bin/env python3
"""Timing of the two-set threshold calls on one MI355X (profiles/r08_a_cross_edges_timing.txt).

    python tools/cross_edges_time.py [--reps 5] [--host-rows 50000] [--out FILE]     the timings
    python tools/cross_edges_time.py --kernels-only                                   three calls of the device route, for a kernel trace
    python tools/cross_edges_time.py --kernel-stats CSV [--out FILE]                  per-kernel times of such a trace (rocprofv3
                                                                                      --kernel-trace --stats) as bytes / s, appended to FILE

h3n2-like 20-mers, k = 4, n_hash = 500, seed 12345.  Host clock around calls that end in a device synchronise, 2 warm-up calls, --reps timed
calls per leg, the legs of a comparison alternated in one process; every leg is reported as min / median / max.

  a  host boundary, m x 100 000: similarityMH_cross_edges at threshold = 0.5 and at thresh_p = 0.99 against the parent path, similarityMH_cross
     (the m x n float64 matrix to the host) followed by the host-side np.nonzero of the thresholded matrix (timed once).
  b  device, 50 000 x 50 000: device.similarity_mh_cross_edges (both forms, into buffers sized by an untimed call with capacity = 0, so that a
     timed call is ONE run of the C route) against device.similarity_mh_cross alone.
  c  the box's streaming rate (a device copy of 8 GiB), the yardstick for the histogram / count / emit kernels' pass over the uint16 block.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, N_HASH, SEED = 4, 500, 12345
DEV_ROWS = 50000
KERNELS = ("k_rect_histogram", "k_threshold_count", "k_threshold_emit")


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"min": float(a[0]), "median": float(np.median(a)), "max": float(a[-1]), "reps": len(a)}


def fmt(s):
    return "min %10.3f  median %10.3f  max %10.3f ms  (%d reps)" % (s["min"], s["median"], s["max"], s["reps"])


def alternate(torch, legs, reps, warm=2):
    out = {k: [] for k in legs}
    for r in range(warm + reps):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warm:
                out[name].append((time.perf_counter() - t) * 1e3)
    return {k: stats(v) for k, v in out.items()}


def kernel_stats(path, out):
    """average time of the three kernels in a rocprofv3 kernel-stats CSV -> the rate of their pass over the DEV_ROWS x DEV_ROWS uint16 block"""
    block_bytes = DEV_ROWS * (-(-DEV_ROWS // 8) * 8) * 2
    lines = ["kernel trace of the device route at %d x %d (one %.2f GB block of uint16 counts per pass)" % (DEV_ROWS, DEV_ROWS, block_bytes / 1e9)]
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            hit = [k for k in KERNELS if k in name]
            if not hit:
                continue
            avg_ns = float(row.get("AverageNs") or row.get("AvgNs") or 0.0)
            calls = int(float(row.get("Calls") or 0))
            lines.append("     %-20s %3d calls, average %9.3f ms -> %.2f TB/s of keys read" %
                         (hit[0], calls, avg_ns / 1e6, block_bytes / max(avg_ns, 1.0) / 1e3))
    print("\n".join(lines), flush=True)
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-rows", type=int, default=50000)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, a.out)
    import torch
    import dynaalign_amd as da
    from dynaalign_amd import device, synth, _capi
    if _capi.load().da_device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured")
    res, off = synth.h3n2_like(100000, 20)
    seqs = synth.to_strings(res, off)
    seeds = da.hash_family_seeds(SEED, N_HASH)
    pack = lambda s: device.DeviceSequences(*da.pack_sequences(s))
    lines, result = [], {}

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    half_x, half_y = pack(seqs[:DEV_ROWS]), pack(seqs[DEV_ROWS:])

    def sized(**kw):
        """the edge count of a form, from a call that stores nothing: the timed calls then run the pipeline once, into buffers that fit"""
        return int(device.similarity_mh_cross_edges(half_x, half_y, K, N_HASH, seeds, capacity=0, **kw)[1][-1].item())
    if a.kernels_only:
        cap = sized(thresh_p=0.99)
        for _ in range(3):
            device.similarity_mh_cross_edges(half_x, half_y, K, N_HASH, seeds, thresh_p=0.99, capacity=cap)
        torch.cuda.synchronize()
        return
    say("two-set threshold form, h3n2-like 20-mers, k = %d, n_hash = %d; 2 warm-up + %d timed calls per leg, legs alternated" % (K, N_HASH, a.reps))
    # c: streaming rate of the box
    src = torch.empty(1 << 30, dtype=torch.int64, device="cuda")
    dst = torch.empty_like(src)
    s = alternate(torch, {"copy": lambda: dst.copy_(src)}, a.reps)["copy"]
    rate = 2 * src.numel() * 8 / (s["median"] * 1e-3) / 1e12
    say("c  device copy of 8 GiB (read + write 16 GiB): %s -> %.2f TB/s" % (fmt(s), rate))
    result["copy"] = {"ms": s, "TB_per_s": rate}
    del src, dst
    torch.cuda.empty_cache()
    # b: device legs
    m, n = half_x.n, half_y.n
    out = torch.empty((m, n), dtype=torch.float64, device="cuda")
    hold = {}
    cap_a, cap_q = sized(threshold=0.5), sized(thresh_p=0.99)
    legs = {"edges, threshold = 0.5 (new)": lambda: hold.__setitem__("a", device.similarity_mh_cross_edges(half_x, half_y, K, N_HASH, seeds, threshold=0.5,
                                                                                                         capacity=cap_a)),
            "edges, thresh_p = 0.99 (new)": lambda: hold.__setitem__("q", device.similarity_mh_cross_edges(half_x, half_y, K, N_HASH, seeds, thresh_p=0.99,
                                                                                                         capacity=cap_q)),
            "dense (parent)": lambda: device.similarity_mh_cross(half_x, half_y, K, N_HASH, seeds, out=out)}
    os.environ["DYNAALIGN_MH_NO_DEDUP"] = "1"              # the dense leg on the direct route too: the same compare on both sides
    r = alternate(torch, legs, a.reps)
    del os.environ["DYNAALIGN_MH_NO_DEDUP"]
    r.update(alternate(torch, {"dense (parent), built-in route": legs["dense (parent)"]}, a.reps))
    say("b  device, %d x %d" % (m, n))
    for k_, v in r.items():
        say("     %-32s %s" % (k_, fmt(v)))
    say("     (threshold = 0.5: %d edges; thresh_p = 0.99: threshold %.3f, %d edges of %d entries)" %
        (hold["a"][2].numel(), hold["q"][0], hold["q"][2].numel(), m * n))
    result["device"] = r
    del out, hold
    torch.cuda.empty_cache()
    _capi.load().da_release_device_memory()
    # a: host boundary
    m = a.host_rows
    x, y = seqs[:m], seqs
    hold = {}
    legs = {"similarityMH_cross_edges, threshold = 0.5 (new)": lambda: hold.__setitem__("a", da.similarityMH_cross_edges(x, y, K, N_HASH, threshold=0.5, seed=SEED)),
            "similarityMH_cross_edges, thresh_p = 0.99 (new)": lambda: hold.__setitem__("q", da.similarityMH_cross_edges(x, y, K, N_HASH, 0.99, seed=SEED)),
            "similarityMH_cross (parent, before thresholding)": lambda: hold.__setitem__("d", da.similarityMH_cross(x, y, K, N_HASH, seed=SEED))}
    r = alternate(torch, legs, a.reps)
    dense = np.asarray(hold["d"])
    t = time.perf_counter()
    i, j = np.nonzero((dense >= 0.5) & (dense > 0))
    nz_ms = (time.perf_counter() - t) * 1e3
    assert np.array_equal(i, hold["a"][1]) and np.array_equal(j, hold["a"][2]), "the two paths disagree"
    say("a  host boundary, %d x %d (%.1f GB of float64 on the parent path)" % (m, len(y), m * len(y) * 8 / 1e9))
    for k_, v in r.items():
        say("     %-52s %s" % (k_, fmt(v)))
    say("     host-side np.nonzero((R >= 0.5) & (R > 0)) of the dense result, one run: %.1f ms" % nz_ms)
    say("     (threshold = 0.5: %d edges; thresh_p = 0.99: threshold %.3f, %d edges; bytes leaving the device: %.3f GB / %.3f GB against %.1f GB "
        "of uint16 counts)" % (len(hold["a"][1]), hold["q"][0], len(hold["q"][1]), len(hold["a"][1]) * 6 / 1e9, len(hold["q"][1]) * 6 / 1e9,
                               m * len(y) * 2 / 1e9))
    result["host"] = {"rows": m, "cols": len(y), "legs": r, "nonzero_ms": nz_ms, "edges_absolute": len(hold["a"][1]), "edges_quantile": len(hold["q"][1])}
    say(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
