#!/usr/bin/env python3
"""Timing of the two-set top-k calls on one MI355X (profiles/r07_a_topk_timing.txt).

    python tools/topk_time.py [--reps 5] [--host-rows 20000] [--out FILE]       the timings
    python tools/topk_time.py --kernels-only                                     three calls of the device route, for a kernel trace

h3n2-like 20-mers, k = 4, n_hash = 500, seed 12345, top = 10.  Host clock around calls that end in a device synchronise, 2 warm-up calls,
--reps timed calls per leg, the legs of a comparison alternated in one process; every leg is reported as min / median / max.

  a  host boundary, m x 100 000: similarityMH_cross_topk against the parent path, similarityMH_cross (the m x n float64 matrix to the host)
     followed by a stable selection on the host (numpy argsort, timed once on --select-rows rows and scaled to m).
  b  device: device.similarity_mh_cross_topk against device.similarity_mh_cross alone, at 50 000 x 50 000 (dictionary codes) and at
     100 000 x 100 000 (the joint operand exceeds 131 068 rows: raw 32-plane compare; the dense result is 80 GB of HBM).
  c  the box's streaming rate (a device copy of 8 GB), the yardstick for the selection kernel's read rate in the kernel trace.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, N_HASH, SEED, TOP = 4, 500, 12345, 10


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-rows", type=int, default=20000)
    ap.add_argument("--select-rows", type=int, default=1000)
    ap.add_argument("--no-full", action="store_true", help="skip the 100 000 x 100 000 device leg")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
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
    half_x, half_y, full = pack(seqs[:50000]), pack(seqs[50000:]), pack(seqs)
    if a.kernels_only:
        for _ in range(3):
            device.similarity_mh_cross_topk(half_x, half_y, K, N_HASH, seeds, TOP)
        torch.cuda.synchronize()
        return
    say("two-set top-k, h3n2-like 20-mers, k = %d, n_hash = %d, top = %d; 2 warm-up + %d timed calls per leg, legs alternated" % (K, N_HASH, TOP, a.reps))
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
    for name, dx, dy, dense_ok in (("50000x50000", half_x, half_y, True), ("100000x100000", full, full, not a.no_full)):
        if not dense_ok:
            continue
        m, n = dx.n, dy.n
        out = torch.empty((m, n), dtype=torch.float64, device="cuda")
        legs = {"topk (new)": lambda: device.similarity_mh_cross_topk(dx, dy, K, N_HASH, seeds, TOP),
                "dense (parent)": lambda: device.similarity_mh_cross(dx, dy, K, N_HASH, seeds, out=out)}
        os.environ["DYNAALIGN_MH_NO_DEDUP"] = "1"              # the dense leg on the direct route too: the same compare on both sides
        r = alternate(torch, legs, a.reps)
        del os.environ["DYNAALIGN_MH_NO_DEDUP"]
        legs2 = {"dense (parent), built-in route": legs["dense (parent)"]}
        r.update(alternate(torch, legs2, a.reps))
        route = device.mh_cross_last_route()
        say("b  device, %s" % name)
        for k_, v in r.items():
            say("     %-32s %s" % (k_, fmt(v)))
        say("     (built-in dense route: dedup = %s, plane bits = %d)" % (route["dedup"], route["plane_bits"]))
        result["device " + name] = r
        del out
        torch.cuda.empty_cache()
        _capi.load().da_release_device_memory()
    # a: host boundary
    m = a.host_rows
    x, y = seqs[:m], seqs
    hold = {}
    legs = {"similarityMH_cross_topk (new)": lambda: hold.__setitem__("t", da.similarityMH_cross_topk(x, y, K, N_HASH, TOP, seed=SEED)),
            "similarityMH_cross (parent, before selection)": lambda: hold.__setitem__("d", da.similarityMH_cross(x, y, K, N_HASH, seed=SEED))}
    r = alternate(torch, legs, a.reps)
    dense = np.asarray(hold["d"])
    t = time.perf_counter()
    sel = np.argsort(-dense[:a.select_rows], axis=1, kind="stable")[:, :TOP]
    sel_ms = (time.perf_counter() - t) * 1e3
    assert np.array_equal(sel, hold["t"][0][:a.select_rows]), "the two paths disagree"
    say("a  host boundary, %d x %d (%.1f GB of float64 on the parent path)" % (m, len(y), m * len(y) * 8 / 1e9))
    for k_, v in r.items():
        say("     %-48s %s" % (k_, fmt(v)))
    say("     host-side stable selection (numpy argsort, %d rows, one run): %.1f ms -> %.1f ms scaled to %d rows" %
        (a.select_rows, sel_ms, sel_ms * m / a.select_rows, m))
    result["host"] = {"rows": m, "cols": len(y), "legs": r, "select_ms_measured_rows": a.select_rows, "select_ms": sel_ms,
                      "select_ms_scaled": sel_ms * m / a.select_rows}
    say(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
