#!/usr/bin/env python3
"""Timing of the device Louvain against the host Louvain step on one MI355X (profiles/r23_a_louvain_device_timing.txt).

    python tools/louvain_time.py [--reps 5] [--n 100000] [--no-recursion] [--no-ladder] [--one-call] [--out FILE]

h3n2-like 20-mers, k = 4, n_hash = 500, seed 12345.  Host clock around calls that end in a device synchronise, 1 warm-up call, --reps timed
calls per leg, the legs of a comparison alternated in one process; every leg is reported as min / median / max.

  a  the first-level graph at thresh_p = .8 (MinHashSession.edges_csr(on_device=True)): device.louvain_csr on the resident CSR against
     the host path of the parent commit -- the device-to-host copy of the CSR plus louvain_csr -- and the modularity of both
  b  the same on the first-level graph at knn = 15
  c  the whole recursion, clusterbreak(size_max=800, session=s) with thresh_p = .8 and with knn = 15, louvain="host" against "device"
  d  the ladder: levels of 10^3 .. 10^7 adjacency entries (the first m sequences), device against host, to place louvain_device_min_nnz

--one-call runs a single device.louvain_csr on graph a and nothing else: the run to put under a kernel trace for the time per kernel.
The device and the host Louvain are different clustering functions: their memberships differ and no parity is claimed.
Expectation to confirm or refute: the device call is several times faster than the host step on graph a.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, N_HASH, SEED = 4, 500, 12345


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
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--no-recursion", action="store_true", help="skip leg c")
    ap.add_argument("--no-ladder", action="store_true", help="skip leg d")
    ap.add_argument("--one-call", action="store_true", help="one device.louvain_csr on graph a, nothing else")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import dynaalign_amd as da
    from dynaalign_amd import device, session, synth, _capi
    from dynaalign_amd.clusterbreak import louvain_csr
    if _capi.load().da_device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured")
    seqs = synth.to_strings(*synth.h3n2_like(a.n, 20))
    s = session.MinHashSession(seqs, K, N_HASH, seed=SEED)
    lines, result = [], {}

    def say(t=""):
        print(t, flush=True)
        lines.append(t)

    def host_step(ptr, adj, codes, loops, values, seed, keep):
        h = (ptr.cpu().numpy(), adj.cpu().numpy(), codes.cpu().numpy().view(np.uint16), loops.cpu().numpy().view(np.uint16))
        keep["host"] = louvain_csr(len(h[0]) - 1, *h, values, seed=seed, return_modularity=True)

    def device_step(ptr, adj, codes, loops, values, seed, keep):
        keep["device"] = device.louvain_csr(ptr, adj, codes, loops, values, seed=seed)

    def compare(tag, csr, reps):
        thr, n_edges, ptr, adj, codes, loops, values = csr
        keep = {}
        r = alternate(torch, {"device.louvain_csr on the resident CSR": lambda: device_step(ptr, adj, codes, loops, values, 1, keep),
                              "host: CSR device -> host + louvain_csr": lambda: host_step(ptr, adj, codes, loops, values, 1, keep)}, reps)
        deg = np.diff(ptr.cpu().numpy())
        m, q, levels, its = keep["device"]
        say("%s: n = %d, %d adjacency entries, largest row %d, workspace %.2f GB" % (tag, len(deg), int(adj.numel()), int(deg.max()) if len(deg) else 0,
                                                                                   device.louvain_workspace_bytes(len(deg), int(adj.numel())) / 1e9))
        for k_, v in r.items():
            say("     %-46s %s" % (k_, fmt(v)))
        say("     device: Q = %.6f, %d communities, %d levels, iterations %s;  host: Q = %.6f, %d communities;  host / device time %.2f"
            % (q, int(m.max()), levels, its, keep["host"][1], int(keep["host"][0].max()),
               r["host: CSR device -> host + louvain_csr"]["median"] / r["device.louvain_csr on the resident CSR"]["median"]))
        result[tag] = {"n": len(deg), "nnz": int(adj.numel()), "timing": r, "device_Q": q, "host_Q": keep["host"][1], "levels": levels, "iterations": its}
        return r

    if a.one_call:
        csr = s.edges_csr(None, .8, on_device=True)
        device.louvain_csr(*csr[2:], seed=1)
        torch.cuda.synchronize()
        return
    say("device Louvain against the host Louvain step, h3n2-like 20-mers, k = %d, n_hash = %d, N = %d; 1 warm-up + %d timed calls per leg, legs alternated"
        % (K, N_HASH, a.n, a.reps))
    csr = s.edges_csr(None, .8, on_device=True)
    compare("a  first level, thresh_p = .8", csr, a.reps)
    del csr
    torch.cuda.empty_cache()
    csr = s.knn_csr_device(None, 15)
    compare("b  first level, knn = 15", csr, a.reps)
    del csr
    torch.cuda.empty_cache()
    if not a.no_recursion:
        say("c  clusterbreak(size_max=800, session=s), end to end")
        for name, kw in (("thresh_p=.8", {"thresh_p": 0.8}), ("knn=15", {"knn": 15})):
            outs = {}

            def run(which):
                outs[which] = da.clusterbreak(seqs, size_max=800, session=s, louvain=which, **kw)
            r = alternate(torch, {"host": lambda: run("host"), "device": lambda: run("device")}, a.reps)
            for which in ("host", "device"):
                o = outs[which]
                say("     %-12s louvain=%-7s %s  calls %d, Louvain %.3f s, graph %.3f s, clustered %d, filtered %d"
                    % (name, which, fmt(r[which]), o.calls, sum(l["cluster_s"] for l in o.levels), sum(l["similarity_s"] for l in o.levels),
                       len(o["clustered_seq"]), len(o["filtered_seq"])))
            result["c " + name] = r
    if not a.no_ladder:
        say("d  ladder: the first m sequences at thresh_p = .8")
        for m in (70, 224, 707, 1250, 2236, 4000, 7071, 12000):
            if m > a.n:
                break
            compare("d  m = %d" % m, s.edges_csr(np.arange(m, dtype=np.int64), .8, on_device=True), a.reps)
    say(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
