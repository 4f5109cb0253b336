#!/usr/bin/env python3
"""Timing of the one-set nearest-neighbour calls on one MI355X (profiles/r14_a_knn_timing.txt).

    python tools/knn_time.py [--reps 5] [--no-full] [--no-cluster] [--out FILE]

h3n2-like 20-mers, k = 4, n_hash = 500, seed 12345, top = 10.  Host clock around calls that end in a device synchronise, 2 warm-up calls,
--reps timed calls per leg, the legs of a comparison alternated in one process; every leg is reported as min / median / max.

  a  similarityMH_knn at the host boundary and device.similarity_mh_knn (the one-call device route) on 50 000 and on 100 000 sequences
  b  in the same run, similarityMH_cross_topk(x, x, top = 11) and device.similarity_mh_cross_topk(x, x, 11): the calls this replaces (their
     result is NOT the lists: among equal values a row's own column is not the first).  Expectation to confirm or refute: a is no slower
     than b -- one K1 pass and an operand of n rows instead of 2n + padding
  c  clusterbreak(size_max=800, session=s, knn=15) against clusterbreak(size_max=800, thresh_p=.8, session=s) on the same 100 000
     sequences: edge counts of the first level, time in Louvain, end to end.  The memberships differ by construction: no parity claim.
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
    ap.add_argument("--no-full", action="store_true", help="skip the 100 000-sequence legs of a / b")
    ap.add_argument("--no-cluster", action="store_true", help="skip leg c")
    ap.add_argument("--cluster-n", type=int, default=100000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import dynaalign_amd as da
    from dynaalign_amd import device, session, synth, _capi
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
    say("one-set nearest-neighbour lists, h3n2-like 20-mers, k = %d, n_hash = %d, top = %d; 2 warm-up + %d timed calls per leg, legs alternated"
        % (K, N_HASH, TOP, a.reps))
    for n in (50000,) if a.no_full else (50000, 100000):
        x = seqs[:n]
        dx = pack(x)
        legs = {"a  device.similarity_mh_knn": lambda: device.similarity_mh_knn(dx, K, N_HASH, seeds, TOP),
                "b  device.similarity_mh_cross_topk(x, x, top + 1)": lambda: device.similarity_mh_cross_topk(dx, dx, K, N_HASH, seeds, TOP + 1),
                "a  similarityMH_knn (host boundary)": lambda: da.similarityMH_knn(x, K, N_HASH, TOP, seed=SEED),
                "b  similarityMH_cross_topk(x, x, top + 1) (host boundary)": lambda: da.similarityMH_cross_topk(x, x, K, N_HASH, TOP + 1, seed=SEED)}
        r = alternate(torch, legs, a.reps)
        say("n = %d" % n)
        for k_, v in r.items():
            say("     %-60s %s" % (k_, fmt(v)))
        result["n=%d" % n] = r
        del dx
        torch.cuda.empty_cache()
        _capi.load().da_release_device_memory()
    if not a.no_cluster:
        pep = seqs[:a.cluster_n]
        s = session.MinHashSession(pep, K, N_HASH, seed=SEED)
        say("c  clusterbreak(size_max=800) on %d sequences, one run each" % len(pep))
        for name, kw in (("knn=15", {"knn": 15}), ("thresh_p=.8", {"thresh_p": 0.8})):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = da.clusterbreak(pep, size_max=800, session=s, **kw)
            total = time.perf_counter() - t
            lv = out.levels
            rec = {"end_to_end_s": total, "calls": out.calls, "first_level_edges": lv[0]["edges"], "edges_all_levels": int(sum(l["edges"] for l in lv)),
                   "similarity_s": float(sum(l["similarity_s"] for l in lv)), "louvain_s": float(sum(l["cluster_s"] for l in lv)),
                   "clustered": int(len(out["clustered_seq"])), "filtered": int(len(out["filtered_seq"]))}
            say("     %-12s end to end %.3f s, Louvain %.3f s, graph %.3f s, calls %d, first-level edges %d, all levels %d, clustered %d, filtered %d"
                % (name, total, rec["louvain_s"], rec["similarity_s"], out.calls, rec["first_level_edges"], rec["edges_all_levels"], rec["clustered"],
                   rec["filtered"]))
            result["clusterbreak " + name] = rec
        say("     (the memberships of the two runs differ by construction: they cluster different graphs)")
    say(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
