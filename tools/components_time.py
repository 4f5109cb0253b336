#!/usr/bin/env python3
"""Timing of the connected components on one MI355X (profiles/r25_a_components_timing.txt).

    python tools/components_time.py [--reps 5] [--sizes 100000,1000000] [--csr-n 20000] [--trace-sizes 100000] [--out FILE]     the timings
    python tools/components_time.py --kernels-only --n N --bands B --rows R                 one warm-up + one traced device.lsh_components call
        (what the tool itself runs under `rocprofv3 --kernel-trace --output-format csv -d DIR --`, a process of its own, for k_lsh_verify's share)

Input: the inputs of tools/lsh_edges_time.py -- synth.h3n2_like(n, 20) made distinct, k = 4, n_hash = 500, seed 12345, threshold 0.5, bands x
rows of 100 x 5 and 50 x 10.  Host clock around calls that end in a device synchronise; one run, 1 warm-up round, then --reps rounds in
which the legs ALTERNATE; min / median / max per leg.

  per size and banding:
    1  device.lsh_components on the resident signatures: n labels cross to the host
    2  the only way to the same labels without it: device.lsh_edges (buffers sized by an untimed call), the edge list to the host,
       da_components there -- and at the host boundary similarityMH_lsh_components against similarityMH_lsh_edges + da_components
  once, at --csr-n drawn (the quantile graph needs the n x n counts, and keeps a fifth of all pairs):
    3  device.components_csr on the tensors of MinHashSession.edges_csr(thresh_p = 0.8, on_device = True) against the copy of that CSR to
       the host + da_components on its entries
  Every leg's labels are compared with leg 1's before anything is timed.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import lsh_edges_time as L  # noqa: E402  (the inputs, the resident signatures, the statistics and their format)

K, N_HASH, SEED, THRESHOLD, BANDINGS = L.K, L.N_HASH, L.SEED, L.THRESHOLD, L.BANDINGS


def alternated(torch, legs, reps, warm=1):
    """legs: name -> callable; every round runs each leg once, in order; -> name -> stats"""
    ms = {name: [] for name in legs}
    for r in range(warm + reps):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warm:
                ms[name].append((time.perf_counter() - t) * 1e3)
    return {name: L.stats(v) for name, v in ms.items()}


def kernels_only(n, bands, rows):
    import torch
    from dynaalign_amd import device
    sig = L.resident_signatures(L.distinct_strings(n))
    device.lsh_components(sig, N_HASH, bands, rows, THRESHOLD)                    # warms up
    torch.cuda.synchronize()
    device.lsh_components(sig, N_HASH, bands, rows, THRESHOLD)                    # the traced call: the last k_lsh_band_keys ... k_cc_label
    torch.cuda.synchronize()


def route_from_trace(trace_dir):
    """device time per kernel family of the LAST pipeline run in a rocprofv3 kernel trace (ms)"""
    import csv
    import glob
    rows = []
    for f in sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)):
        for r in csv.DictReader(open(f)):
            k = {key.lower(): v for key, v in r.items()}
            rows.append((int(k["start_timestamp"]), int(k["end_timestamp"]), k["kernel_name"]))
    rows.sort()
    starts = [t for t, r in enumerate(rows) if "k_lsh_band_keys" in r[2]]
    if not starts:
        return None
    out = {"all kernels": 0.0, "k_lsh_verify": 0.0, "k_lsh_union": 0.0, "k_cc_*": 0.0}
    for b, e, name in rows[starts[-1]:]:
        d = (e - b) * 1e-6
        out["all kernels"] += d
        for key in ("k_lsh_verify", "k_lsh_union"):
            if key in name:
                out[key] += d
        if "k_cc_" in name:
            out["k_cc_*"] += d
    return out


def trace_route(n, bands, rows):
    """one device.lsh_components call under rocprofv3 --kernel-trace in a child process of its own"""
    d = tempfile.mkdtemp(prefix="cc_trace_")
    try:
        print("tracing one device.lsh_components call at n = %d, %d x %d ..." % (n, bands, rows), file=sys.stderr, flush=True)
        cmd = [shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--kernels-only", "--n", str(n), "--bands", str(bands), "--rows", str(rows)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
        except subprocess.TimeoutExpired as e:
            # a traced child that hangs ends the tool: nothing more is started on the GPU
            raise SystemExit("the traced child at n = %d, %d x %d did not end within 240 s; nothing more is run\n%s"
                             % (n, bands, rows, (e.output or b"").decode("latin-1")[-4000:]))
        if p.returncode != 0:
            sys.stderr.write(p.stdout.decode("latin-1")[-4000:])
            raise SystemExit("the traced child at n = %d, %d x %d ended with status %d; nothing more is run" % (n, bands, rows, p.returncode))
        return route_from_trace(d)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def csr_to_edges_host(ptr, adj):
    """the host's half of leg 3: the device CSR copied over and its entries with adj > row as an edge list"""
    ptr, adj = ptr.cpu().numpy(), adj.cpu().numpy()
    rows = np.repeat(np.arange(len(ptr) - 1, dtype=np.int32), np.diff(ptr))
    up = adj > rows
    return rows[up], adj[up]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--csr-n", type=int, default=20000)
    ap.add_argument("--trace-sizes", default="100000")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--bands", type=int, default=100)
    ap.add_argument("--rows", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.kernels_only:
        return kernels_only(a.n, a.bands, a.rows)
    sizes = [int(s) for s in a.sizes.split(",") if s]
    traced = [int(s) for s in a.trace_sizes.split(",") if s]
    traces = {}
    for n in sizes:                                           # the children first: this process has not opened the GPU yet
        if n in traced:
            for bands, rows in BANDINGS:
                traces[(n, bands, rows)] = trace_route(n, bands, rows)
    import torch
    import dynaalign_amd as da
    from dynaalign_amd import device, session, _capi
    if _capi.load().da_device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured")
    lines, result = [], []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say("Connected components, h3n2-like 20-mers made distinct, k = %d, n_hash = %d, seed %d, threshold %.2f; one run, 1 warm-up round + %d rounds, "
        "legs alternated" % (K, N_HASH, SEED, THRESHOLD, a.reps))
    for n in sizes:
        seqs = L.distinct_strings(n)
        m = len(seqs)
        sig = L.resident_signatures(seqs)
        say("n = %d drawn, %d distinct" % (n, m))
        for bands, rows in BANDINGS:
            rec = {"n": m, "bands": bands, "rows": rows}
            try:
                member, count = device.lsh_components(sig, N_HASH, bands, rows, THRESHOLD)
            except da.DynaAlignError as e:
                say("  %3d x %2d: refused: %s" % (bands, rows, e))
                continue
            route = device.mh_lsh_last_route()
            cap = device.lsh_edges(sig, N_HASH, bands, rows, THRESHOLD)[0].numel()
            hold = {}

            def leg2_device():
                ei, ej, _ = device.lsh_edges(sig, N_HASH, bands, rows, THRESHOLD, capacity=cap)
                hold["dev"] = da.components(m, ei.cpu().numpy(), ej.cpu().numpy(), return_count=True)

            def leg2_host():
                _, ei, ej, _ = da.similarityMH_lsh_edges(seqs, K, N_HASH, bands, rows, THRESHOLD, seed=SEED)
                hold["host"] = da.components(m, ei, ej, return_count=True)
            legs = {
                "1  device.lsh_components": lambda: device.lsh_components(sig, N_HASH, bands, rows, THRESHOLD),
                "2  device.lsh_edges + edges to host + da_components": leg2_device,
                "1h similarityMH_lsh_components (host boundary)": lambda: hold.__setitem__("h1", da.similarityMH_lsh_components(seqs, K, N_HASH, bands, rows, THRESHOLD, seed=SEED)),
                "2h similarityMH_lsh_edges + da_components (host boundary)": leg2_host,
            }
            for fn in legs.values():                          # the labels first: every leg gives leg 1's
                fn()
            for key in ("dev", "host", "h1"):
                assert hold[key][1] == count and np.array_equal(hold[key][0], member), "the legs disagree (%s)" % key
            sizes_c = np.bincount(member)[1:]
            say("  %3d bands x %2d rows: %d buckets, %d incidences, %d distinct candidate pairs, %d edges (diagonal included) -> %d components, "
                "the largest of %d, %d singletons" % (bands, rows, route["buckets"], route["incidences"], route["verified_pairs"], route["edges"], count,
                                                      int(sizes_c.max()), int((sizes_c == 1).sum())))
            t = alternated(torch, legs, a.reps)
            for name, s in t.items():
                say("      %-58s %s" % (name, L.fmt(s)))
            say("      leg 2 / leg 1 (medians): device boundary %.2f x, host boundary %.2f x"
                % (t["2  device.lsh_edges + edges to host + da_components"]["median"] / t["1  device.lsh_components"]["median"],
                   t["2h similarityMH_lsh_edges + da_components (host boundary)"]["median"] / t["1h similarityMH_lsh_components (host boundary)"]["median"]))
            rec.update(route=route, components=count, ms=t)
            st = traces.get((n, bands, rows))
            if st:
                say("      kernel trace of one device.lsh_components call: all kernels %.3f ms; k_lsh_verify %.3f ms = %.1f %%; k_lsh_union %.3f ms; "
                    "k_cc_* %.3f ms" % (st["all kernels"], st["k_lsh_verify"], 100.0 * st["k_lsh_verify"] / max(st["all kernels"], 1e-9), st["k_lsh_union"],
                                        st["k_cc_*"]))
                rec["trace_ms"] = st
            result.append(rec)
            del hold
        del sig
        torch.cuda.empty_cache()
        _capi.load().da_release_device_memory()
    if a.csr_n > 0:
        seqs = L.distinct_strings(a.csr_n)
        m = len(seqs)
        s = session.MinHashSession(seqs, K, N_HASH, seed=SEED)
        thr, got, ptr, adj, _, _, _ = s.edges_csr(None, 0.8, on_device=True)
        member, count = device.components_csr(ptr, adj)
        hold = {}

        def leg3_host():
            ei, ej = csr_to_edges_host(ptr, adj)
            hold["host"] = da.components(m, ei, ej, return_count=True)
        legs = {"3  device.components_csr": lambda: device.components_csr(ptr, adj),
                "3h CSR to host + da_components": leg3_host}
        leg3_host()
        assert hold["host"][1] == count and np.array_equal(hold["host"][0], member), "the legs disagree (csr)"
        say("quantile graph of %d drawn, %d distinct, thresh_p = 0.8: threshold %.4f, %d edges (i <= j), %d adjacency entries -> %d components"
            % (a.csr_n, m, thr, got, adj.numel(), count))
        t = alternated(torch, legs, a.reps)
        for name, st in t.items():
            say("      %-58s %s" % (name, L.fmt(st)))
        say("      leg 3h / leg 3 (medians): %.2f x" % (t["3h CSR to host + da_components"]["median"] / t["3  device.components_csr"]["median"]))
        result.append({"csr_n": m, "edges": int(got), "components": count, "ms": t})
    say(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
