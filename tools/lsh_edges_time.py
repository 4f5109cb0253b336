#!/usr/bin/env python3
"""Timing of MinHash LSH banding on one MI355X (profiles/r20_a_lsh_edges_timing.txt).

    python tools/lsh_edges_time.py [--reps 3] [--sizes 100000,1000000] [--no-trace] [--out FILE]     the timings
    python tools/lsh_edges_time.py --kernels-only --n N --bands B --rows R                           one warm-up + one traced device call
        (what the tool itself runs under `rocprofv3 --kernel-trace --output-format csv -d DIR --`, a process of its own, for the stages)

Input: synth.h3n2_like(n, 20) made distinct (first occurrences, in order); k = 4, n_hash = 500, seed 12345, threshold 0.5, bands x rows of
100 x 5 and 50 x 10.  Host clock around calls that end in a device synchronise, 1 warm-up call, --reps timed calls, min / median / max.

  per size and banding:
    device   device.lsh_edges on the resident signatures (buffers sized by an untimed call): bucketing, verification, emit + sort
    host     similarityMH_lsh_edges on the strings: upload, signatures, the same pipeline, the edge list to the host
    stages   from the kernel trace of one device call: 1 keys + sort + runs + partner counts, 2 k_lsh_verify + the chunk scan,
             3 diagonal + emit + sort + split; the verify kernel's rate in pairs / s and bytes of signature rows / s
    counts   buckets, (pair, band) incidences, distinct candidate pairs, edges
  at the first size only: similarityMH_cross_edges(x, x, threshold=0.5) on the same seed -- the all-pairs graph -- timed in the same run, and the
  recall of the LSH edge list against its upper triangle.
"""
import argparse
import csv
import glob
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

K, N_HASH, SEED, THRESHOLD = 4, 500, 12345, 0.5
BANDINGS = ((100, 5), (50, 10))


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"min": float(a[0]), "median": float(np.median(a)), "max": float(a[-1]), "reps": len(a)}


def fmt(s):
    return "min %10.3f  median %10.3f  max %10.3f ms  (%d reps)" % (s["min"], s["median"], s["max"], s["reps"])


def timed(torch, fn, reps, warm=1):
    out = []
    for r in range(warm + reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warm:
            out.append((time.perf_counter() - t) * 1e3)
    return stats(out)


def distinct_strings(n):
    from dynaalign_amd import synth
    res, off = synth.h3n2_like(n, 20)
    return list(dict.fromkeys(synth.to_strings(res, off)))


def resident_signatures(seqs):
    import dynaalign_amd as da
    from dynaalign_amd import device
    ds = device.DeviceSequences(*da.pack_sequences(seqs))
    sig, _ = device.minhash_signatures(ds, K, N_HASH, da.hash_family_seeds(SEED, N_HASH), want_planes=False)
    return sig


def kernels_only(n, bands, rows):
    import torch
    from dynaalign_amd import device
    sig = resident_signatures(distinct_strings(n))
    cap = device.lsh_edges(sig, N_HASH, bands, rows, THRESHOLD)[0].numel()        # sizes the buffers (and warms up)
    torch.cuda.synchronize()
    device.lsh_edges(sig, N_HASH, bands, rows, THRESHOLD, capacity=cap)           # the traced call: the last k_lsh_band_keys ... k_lsh_split
    torch.cuda.synchronize()


def stages_from_trace(trace_dir):
    """device time of the three stages of the LAST pipeline run in a rocprofv3 kernel trace (ms), and the verify kernel alone"""
    rows = []
    for f in sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)):
        for r in csv.DictReader(open(f)):
            k = {key.lower(): v for key, v in r.items()}
            rows.append((int(k["start_timestamp"]), int(k["end_timestamp"]), k["kernel_name"]))
    rows.sort()
    starts = [t for t, r in enumerate(rows) if "k_lsh_band_keys" in r[2]]
    if not starts:
        return None
    rows = rows[starts[-1]:]
    out = {"bucketing": 0.0, "verify": 0.0, "emit + sort": 0.0, "k_lsh_verify": 0.0}
    stage = "bucketing"
    for b, e, name in rows:
        if "k_lsh_verify" in name:
            stage = "verify"
            out["k_lsh_verify"] += (e - b) * 1e-6
        elif "k_lsh_diagonal" in name:
            stage = "emit + sort"
        out[stage] += (e - b) * 1e-6
    return out


def trace_stages(n, bands, rows):
    """one device call under rocprofv3 --kernel-trace in a child process of its own"""
    d = tempfile.mkdtemp(prefix="lsh_trace_")
    try:
        print("tracing one device call at n = %d, %d x %d ..." % (n, bands, rows), file=sys.stderr, flush=True)
        cmd = [shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--kernels-only",
               "--n", str(n), "--bands", str(bands), "--rows", str(rows)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
        except subprocess.TimeoutExpired as e:
            # a traced child that hangs ends the tool: nothing more is started on the GPU
            raise SystemExit("the traced child at n = %d, %d x %d did not end within 240 s; nothing more is run\n%s"
                             % (n, bands, rows, (e.output or b"").decode("latin-1")[-4000:]))
        if p.returncode != 0:
            # so does one that fails, whatever the reason (a refused cap, a HIP error, an abort, a fault): its output says which
            sys.stderr.write(p.stdout.decode("latin-1")[-4000:])
            raise SystemExit("the traced child at n = %d, %d x %d ended with status %d; nothing more is run" % (n, bands, rows, p.returncode))
        return stages_from_trace(d)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--bands", type=int, default=100)
    ap.add_argument("--rows", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.kernels_only:
        return kernels_only(a.n, a.bands, a.rows)
    sizes = [int(s) for s in a.sizes.split(",")]
    traces = {}
    if not a.no_trace:                                     # the children first: this process has not opened the GPU yet
        for n in sizes:
            for bands, rows in BANDINGS:
                traces[(n, bands, rows)] = trace_stages(n, bands, rows)
    import torch
    import dynaalign_amd as da
    from dynaalign_amd import device, similarity, _capi
    if _capi.load().da_device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured")
    lines, result = [], []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say("MinHash LSH banding, h3n2-like 20-mers made distinct, k = %d, n_hash = %d, seed %d, threshold %.2f; 1 warm-up + %d timed calls"
        % (K, N_HASH, SEED, THRESHOLD, a.reps))
    for pos, n in enumerate(sizes):
        seqs = distinct_strings(n)
        m = len(seqs)
        sig = resident_signatures(seqs)
        say("n = %d drawn, %d distinct" % (n, m))
        all_pairs = None
        if pos == 0:
            hold = {}
            s = timed(torch, lambda: hold.__setitem__("e", da.similarityMH_cross_edges(seqs, seqs, K, N_HASH, threshold=THRESHOLD, seed=SEED)), a.reps)
            _, ai, aj, _ = hold["e"]
            up = ai <= aj
            all_pairs = np.unique(ai[up].astype(np.int64) << 32 | aj[up].astype(np.int64))
            say("  all pairs: similarityMH_cross_edges(x, x, threshold = %.2f), host boundary  %s; %d edges with i <= j" % (THRESHOLD, fmt(s), len(all_pairs)))
            result.append({"n": m, "all_pairs_ms": s, "all_pairs_edges": int(len(all_pairs))})
            del hold
        for bands, rows in BANDINGS:
            rec = {"n": m, "bands": bands, "rows": rows}
            try:
                ei, ej, _ = device.lsh_edges(sig, N_HASH, bands, rows, THRESHOLD)
            except da.DynaAlignError as e:
                say("  %3d x %2d: refused: %s" % (bands, rows, e))
                continue
            cap = ei.numel()
            route = similarity.mh_lsh_last_route()
            dev = timed(torch, lambda: device.lsh_edges(sig, N_HASH, bands, rows, THRESHOLD, capacity=cap), a.reps)
            hold = {}
            host = timed(torch, lambda: hold.__setitem__("e", da.similarityMH_lsh_edges(seqs, K, N_HASH, bands, rows, THRESHOLD, seed=SEED)), a.reps)
            _, hi, hj, _ = hold["e"]
            assert np.array_equal(hi, ei.cpu().numpy()) and np.array_equal(hj, ej.cpu().numpy()), "host and device routes disagree"
            say("  %3d bands x %2d rows: %d buckets, %d incidences, %d distinct candidate pairs, %d edges (diagonal included)"
                % (bands, rows, route["buckets"], route["incidences"], route["verified_pairs"], route["edges"]))
            say("      device  %s" % fmt(dev))
            say("      host    %s" % fmt(host))
            rec.update(route=route, device_ms=dev, host_ms=host)
            st = traces.get((n, bands, rows))
            if st:
                rate = route["incidences"] / max(st["k_lsh_verify"], 1e-9) * 1e3
                say("      stages (kernel trace of one device call): bucketing %.3f ms, verify %.3f ms, emit + sort %.3f ms; k_lsh_verify alone %.3f ms = "
                    "%.3g pairs/s = %.2f TB/s of signature rows" % (st["bucketing"], st["verify"], st["emit + sort"], st["k_lsh_verify"], rate,
                                                                     rate * 2 * N_HASH * 4 / 1e12))
                rec["stages_ms"] = st
            elif not a.no_trace:
                say("      stages: the trace holds no k_lsh_band_keys launch")
            if all_pairs is not None:
                lsh = hi.astype(np.int64) << 32 | hj.astype(np.int64)
                hit = int(np.isin(all_pairs, lsh, assume_unique=True).sum())
                extra = int(len(lsh) - np.isin(lsh, all_pairs, assume_unique=True).sum())
                say("      recall against the all-pairs graph: %d of %d edges = %.4f (%d LSH edges are not in it)" % (hit, len(all_pairs), hit / len(all_pairs), extra))
                rec.update(recall=hit / len(all_pairs), all_pairs_edges=int(len(all_pairs)))
            result.append(rec)
            del hold
        del sig
        torch.cuda.empty_cache()
        _capi.load().da_release_device_memory()
    say(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
