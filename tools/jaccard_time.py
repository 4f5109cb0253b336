#!/usr/bin/env python3
"""Timing of the exact Jaccard index against the MinHash estimate it replaces, on one MI355X (profiles/r17_a_jaccard_timing.txt; DESIGN.md
section 7).

    python tools/jaccard_time.py [--reps 3] [--n 50000] [--out FILE] [--exact-only]

Inputs: synth.h3n2_like(n, 20) at k = 4 and n h3n2-like 12-mers at k = 2.  Host clock around calls that end in a device synchronise, 2 warm-up
calls, --reps timed calls per leg, the legs alternated in one process; every leg is reported as min / median / max.

  a  device.jaccard_sets + device.jaccard_rect into uint16 codes for the full square
  b  device.minhash_signatures + device.mh_planes + device.mh_compare(kind = COMPACT) on the same input at n_hash = 50 and 500: the MinHash
     route of the square problem, the code this measure is an alternative to
  c  similarityJaccard_knn against similarityMH_knn (n_hash = 50 and 500), top = 10, at the host boundary

Expectation to confirm or refute: for these short peptides a is no slower than b at n_hash = 500.  --exact-only runs the exact legs alone (a and
c's similarityJaccard_knn): the run to take a kernel trace of (rocprofv3 --kernel-trace --stats -d DIR -- python tools/jaccard_time.py --exact-only).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED, TOP = 12345, 10


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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--exact-only", action="store_true", help="only the exact legs: the run a kernel trace is taken of")
    a = ap.parse_args()
    import torch
    import dynaalign_amd as da
    from dynaalign_amd import device, synth, _capi
    from dynaalign_amd._capi import DA_OUT_COMPACT
    if _capi.load().da_device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured")
    lines, result = [], {}

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say("exact Jaccard against the MinHash estimate, %d sequences, top = %d; 2 warm-up + %d timed calls per leg, legs alternated" % (a.n, TOP, a.reps))
    for label, length, k in (("h3n2-like 20-mers, k = 4", 20, 4), ("h3n2-like 12-mers, k = 2", 12, 2)):
        res, off = synth.h3n2_like(a.n, length)
        seqs = synth.to_strings(res, off)
        ds = device.DeviceSequences(res, off)
        n = ds.n
        out = torch.empty((n, n), dtype=torch.int16, device="cuda")      # one result buffer for every device leg
        seeds = {nh: da.hash_family_seeds(SEED, nh) for nh in (50, 500)}

        def exact():
            device.jaccard_rect(device.jaccard_sets(ds, k), kind=DA_OUT_COMPACT, out=out)

        def sets_only():
            device.jaccard_sets(ds, k)

        def minhash(nh):
            sig, _ = device.minhash_signatures(ds, k, nh, seeds[nh], want_planes=False)
            device.mh_compare(device.mh_planes(sig, n, nh), n, nh, kind=DA_OUT_COMPACT, out=out)
        legs = {"a  jaccard_sets + jaccard_rect (uint16 codes)": exact,
                "a' jaccard_sets alone": sets_only,
                "b  minhash_signatures + mh_planes + mh_compare, n_hash = 50": lambda: minhash(50),
                "b  minhash_signatures + mh_planes + mh_compare, n_hash = 500": lambda: minhash(500),
                "c  similarityJaccard_knn (host boundary)": lambda: da.similarityJaccard_knn(seqs, k, TOP),
                "c  similarityMH_knn, n_hash = 50 (host boundary)": lambda: da.similarityMH_knn(seqs, k, 50, TOP, seed=SEED),
                "c  similarityMH_knn, n_hash = 500 (host boundary)": lambda: da.similarityMH_knn(seqs, k, 500, TOP, seed=SEED)}
        if a.exact_only:
            legs = {name: fn for name, fn in legs.items() if "jaccard" in name.lower()}
        r = alternate(torch, legs, a.reps)
        say(label)
        for name, v in r.items():
            say("     %-62s %s" % (name, fmt(v)))
        result[label] = r
        del out, ds
        torch.cuda.empty_cache()
        _capi.load().da_release_device_memory()
    say(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
