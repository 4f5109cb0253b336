#!/usr/bin/env python3
"""Timing of the Levenshtein similarity against the two order-aware / exact measures beside it, on one MI355X.

    python tools/lev_time.py [--reps 5] [--sets 20:50000,20:100000,60:20000,120:20000] [--host-max-n 100000] [--out FILE] [--lev-only]

Inputs: per LENGTH:N of --sets, synth.h3n2_like(N, LENGTH) made distinct (first occurrences, in order): 20-mers run the one-uint32 kernel,
60-mers the one-uint64 kernel, 120-mers the two-uint64 kernel.  Host clock around calls that end in a device synchronise, 1 warm-up round,
--reps timed rounds, the legs alternated in one process; every leg is reported as min / median / max.

  a  device.lev_masks + device.lev_rect into uint16 codes for the full square (the class map is computed once on the host, outside the timed
     calls); a' device.lev_masks alone; a" device.lev_rect alone on resident masks
  b  device.nw (da_dev_nw, BLOSUM62 10 / 4) into uint16 codes for the full square, on the same sequences
  c  device.jaccard_sets + device.jaccard_rect at k = 4 into uint16 codes for the full square
  d  similarityLev_knn against similarityNW_knn, top = 10, at the host boundary (sets of at most --host-max-n sequences)
  e  similarityLev_edges at thresh_p = 0.999 at the host boundary (the 0.8 of clusterbreak would list a fifth of all pairs: at 100 000
     sequences a billion edges; the quantile pass and the extraction are the same)

Expectation to confirm or refute: the 32-bit square (a on 20-mers) costs several times less than the direct NW sweep (b) on the same 20-mers.
--lev-only runs the Levenshtein legs alone: the run to take a kernel trace of (rocprofv3 --kernel-trace --stats -d DIR -- python
tools/lev_time.py --lev-only).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOP, EDGES_P = 10, 0.999


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"min": float(a[0]), "median": float(np.median(a)), "max": float(a[-1]), "reps": len(a)}


def fmt(s):
    return "min %10.3f  median %10.3f  max %10.3f ms  (%d reps)" % (s["min"], s["median"], s["max"], s["reps"])


def alternate(torch, legs, reps, warm=1):
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
    ap.add_argument("--sets", default="20:50000,20:100000,60:20000,120:20000", help="LENGTH:N, comma-separated")
    ap.add_argument("--host-max-n", type=int, default=100000, help="the host-boundary legs run on sets of at most this many sequences")
    ap.add_argument("--out", default=None)
    ap.add_argument("--lev-only", action="store_true", help="only the Levenshtein legs: the run a kernel trace is taken of")
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
    say("Levenshtein similarity against NW identity and the exact Jaccard index (k = 4), top = %d, edges at thresh_p = %g; 1 warm-up + %d timed "
        "rounds, legs alternated" % (TOP, EDGES_P, a.reps))
    for spec in a.sets.split(","):
        length, drawn = (int(v) for v in spec.split(":"))
        res, off = synth.h3n2_like(drawn, length)
        seqs = list(dict.fromkeys(synth.to_strings(res, off)))
        pres, poff = da.pack_sequences(seqs)
        ds = device.DeviceSequences(pres, poff)
        n = ds.n
        # the byte values that occur, numbered in ascending order: a property of the input like its upload, computed once on the host
        seen = np.bincount(pres[:int(poff[-1])], minlength=256) > 0
        class_map = np.where(seen, np.cumsum(seen) - 1, 0).astype(np.uint8)
        resident = device.lev_masks(ds, class_map)
        label = "h3n2-like %d-mers: %d drawn, %d distinct" % (length, drawn, n)
        out = torch.empty((n, n), dtype=torch.int16, device="cuda")      # one result buffer for every device leg
        device.nw_encode(ds)

        def lev():
            device.lev_rect(device.lev_masks(ds, class_map), kind=DA_OUT_COMPACT, out=out)

        def jaccard():
            device.jaccard_rect(device.jaccard_sets(ds, 4), kind=DA_OUT_COMPACT, out=out)
        legs = {"a  lev_masks + lev_rect (uint16 codes)": lev,
                "a' lev_masks alone": lambda: device.lev_masks(ds, class_map),
                'a" lev_rect alone, on resident masks': lambda: device.lev_rect(resident, kind=DA_OUT_COMPACT, out=out),
                "b  da_dev_nw, BLOSUM62 10 / 4 (uint16 codes)": lambda: device.nw(ds, kind=DA_OUT_COMPACT, out=out),
                "c  jaccard_sets + jaccard_rect, k = 4 (uint16 codes)": jaccard}
        if n <= a.host_max_n:
            legs.update({"d  similarityLev_knn (host boundary)": lambda: da.similarityLev_knn(seqs, TOP),
                         "d  similarityNW_knn (host boundary)": lambda: da.similarityNW_knn(seqs, top=TOP),
                         "e  similarityLev_edges, thresh_p = %g (host boundary)" % EDGES_P: lambda: da.similarityLev_edges(seqs, EDGES_P)})
        if a.lev_only:
            legs = {name: fn for name, fn in legs.items() if "lev" in name.lower()}
        r = alternate(torch, legs, a.reps)
        say(label)
        for name, v in r.items():
            say("     %-62s %s" % (name, fmt(v)))
        result[label] = r
        del out, ds, resident
        torch.cuda.empty_cache()
        _capi.load().da_release_device_memory()
    say(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
