#!/usr/bin/env python3
"""Timing of the LSH nearest-neighbour lists on one MI355X (profiles/r21_a_lsh_knn_timing.txt).

    python tools/lsh_knn_time.py [--reps 5] [--sizes 100000,1000000] [--no-trace] [--out FILE]      the timings
    python tools/lsh_knn_time.py --kernels-only --n N --bands B --rows R                            one warm-up + one traced device call
        (what the tool itself runs under `rocprofv3 --kernel-trace --output-format csv -d DIR --`, a process of its own, for the stages)

Input: synth.h3n2_like(n, 20) made distinct (first occurrences, in order); k = 4, n_hash = 500, seed 12345, top = 10, bands x rows of
100 x 5 and 50 x 10.  Host clock around calls that end in a device synchronise.  The legs of one (size, banding) are timed in ONE run and
ALTERNATED -- round r runs every leg once, in order -- after one warm-up round; min / median / max over --reps rounds.

  per size and banding:
    knn device   device.lsh_knn on the resident signatures: bucketing, verification, degrees + scatter, selection
    knn host     similarityMH_lsh_knn on the strings: upload, signatures, the same pipeline, the lists to the host
    edges device device.lsh_edges(threshold = 0.5) on the same signatures (buffers sized by an untimed call): the threshold form beside it
    stages       from the kernel trace of one device.lsh_knn call: 1 keys + sort + runs + partner counts, 2 k_lsh_verify + the chunk scan,
                 3 k_lsh_knn_entries (degrees, scan, scatter) + k_lsh_knn_written, 4 k_lsh_knn_select_short + _long
    counts       buckets, (pair, band) incidences, distinct candidate pairs, list entries written
  at the first size only, in the same run: similarityMH_knn (host boundary) and device.similarity_mh_knn (all pairs), and recall@10 of the
  LSH lists against similarityMH_knn's, counting only its entries with value > 0.

EXPECTATION, written down before the first measurement: everything after verify (stages 3 + 4) is a minor share of the device call, as emit +
sort is for the edge form (0.46 of 9.6 ms at 44 931 sequences, 100 x 5).  "Minor" is taken as under a quarter of the kernel time at every
measured point; the tool prints the shares and whether that held.
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

K, N_HASH, SEED, TOP, EDGE_THRESHOLD = 4, 500, 12345, 10, 0.5
BANDINGS = ((100, 5), (50, 10))
STAGES = ("bucketing", "verify", "degrees + scatter", "select")


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"min": float(a[0]), "median": float(np.median(a)), "max": float(a[-1]), "reps": len(a)}


def fmt(s):
    return "min %10.3f  median %10.3f  max %10.3f ms  (range %.3f, %d reps)" % (s["min"], s["median"], s["max"], s["max"] - s["min"], s["reps"])


def alternated(torch, legs, reps, warm=1):
    """legs: [(name, fn)].  Round r runs every leg once, in order; the first `warm` rounds are not kept.  -> {name: stats}"""
    out = {name: [] for name, _ in legs}
    for r in range(warm + reps):
        for name, fn in legs:
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warm:
                out[name].append((time.perf_counter() - t) * 1e3)
    return {name: stats(v) for name, v in out.items()}


def distinct_strings(n):
    from dynaalign_amd import synth
    res, off = synth.h3n2_like(n, 20)
    return list(dict.fromkeys(synth.to_strings(res, off)))


def resident(seqs):
    import dynaalign_amd as da
    from dynaalign_amd import device
    ds = device.DeviceSequences(*da.pack_sequences(seqs))
    sig, _ = device.minhash_signatures(ds, K, N_HASH, da.hash_family_seeds(SEED, N_HASH), want_planes=False)
    return ds, sig


def kernels_only(n, bands, rows):
    import torch
    from dynaalign_amd import device
    _, sig = resident(distinct_strings(n))
    device.lsh_knn(sig, N_HASH, bands, rows, TOP)                                 # warms up
    torch.cuda.synchronize()
    device.lsh_knn(sig, N_HASH, bands, rows, TOP)                                 # the traced call: the last k_lsh_band_keys ... k_lsh_knn_select_long
    torch.cuda.synchronize()


def stages_from_trace(trace_dir):
    """device time of the four stages of the LAST pipeline run in a rocprofv3 kernel trace (ms), and the verify kernel alone"""
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
    out = {s: 0.0 for s in STAGES}
    out["k_lsh_verify"] = 0.0
    stage = "bucketing"
    for b, e, name in rows:
        if "k_lsh_verify" in name:
            stage = "verify"
            out["k_lsh_verify"] += (e - b) * 1e-6
        elif "k_lsh_knn_entries" in name or "k_lsh_knn_written" in name:
            stage = "degrees + scatter"
        elif "k_lsh_knn_select" in name:
            stage = "select"
        out[stage] += (e - b) * 1e-6
    return out


def trace_stages(n, bands, rows):
    """one device call under rocprofv3 --kernel-trace in a child process of its own"""
    d = tempfile.mkdtemp(prefix="lsh_knn_trace_")
    try:
        print("tracing one device call at n = %d, %d x %d ..." % (n, bands, rows), file=sys.stderr, flush=True)
        cmd = [shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--kernels-only", "--n", str(n), "--bands", str(bands), "--rows", str(rows)]
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
    ap.add_argument("--reps", type=int, default=5)
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
    lines, result, verdicts = [], [], []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say("LSH nearest-neighbour lists, h3n2-like 20-mers made distinct, k = %d, n_hash = %d, seed %d, top = %d; legs alternated, 1 warm-up + %d timed rounds"
        % (K, N_HASH, SEED, TOP, a.reps))
    say("expectation (stated before measuring): degrees + scatter + select are a minor share of the device call, as emit + sort is for the edge form")
    seeds = da.hash_family_seeds(SEED, N_HASH)
    for pos, n in enumerate(sizes):
        seqs = distinct_strings(n)
        m = len(seqs)
        ds, sig = resident(seqs)
        say("n = %d drawn, %d distinct" % (n, m))
        ref = None
        for bands, rows in BANDINGS:
            rec = {"n": m, "bands": bands, "rows": rows}
            try:
                li, lk = device.lsh_knn(sig, N_HASH, bands, rows, TOP)
                route = similarity.mh_lsh_last_route()
                cap = device.lsh_edges(sig, N_HASH, bands, rows, EDGE_THRESHOLD)[0].numel()
            except da.DynaAlignError as e:
                say("  %3d x %2d: refused: %s" % (bands, rows, e))
                continue
            hold = {}
            legs = [("knn device", lambda: device.lsh_knn(sig, N_HASH, bands, rows, TOP)),
                    ("knn host", lambda: hold.__setitem__("l", da.similarityMH_lsh_knn(seqs, K, N_HASH, bands, rows, TOP, seed=SEED))),
                    ("edges device", lambda: device.lsh_edges(sig, N_HASH, bands, rows, EDGE_THRESHOLD, capacity=cap))]
            if pos == 0:
                legs += [("all-pairs knn host", lambda: hold.__setitem__("r", da.similarityMH_knn(seqs, K, N_HASH, TOP, seed=SEED))),
                         ("all-pairs knn device", lambda: device.similarity_mh_knn(ds, K, N_HASH, seeds, TOP))]
            t = alternated(torch, legs, a.reps)
            hi, hv = hold["l"]
            assert np.array_equal(hi, li.cpu().numpy()), "host and device routes disagree"
            say("  %3d bands x %2d rows: %d buckets, %d incidences, %d distinct candidate pairs, %d list entries (%.2f per row)"
                % (bands, rows, route["buckets"], route["incidences"], route["verified_pairs"], route["edges"], route["edges"] / m))
            for name, _ in legs:
                say("      %-21s %s" % (name, fmt(t[name])))
            rec.update(route=route, ms=t, edge_list_edges=cap)
            st = traces.get((n, bands, rows))
            if st:
                after = st["degrees + scatter"] + st["select"]
                total = sum(st[s] for s in STAGES)
                say("      stages (kernel trace of one device call): bucketing %.3f ms, verify %.3f ms, degrees + scatter %.3f ms, select %.3f ms; "
                    "after verify: %.3f of %.3f ms of kernels = %.1f %%" % (st["bucketing"], st["verify"], st["degrees + scatter"], st["select"], after, total,
                                                                          100.0 * after / total))
                verdicts.append((m, bands, rows, after / total))
                rec["stages_ms"] = st
            elif not a.no_trace:
                say("      stages: the trace holds no k_lsh_band_keys launch")
            if pos == 0:
                ref = hold["r"]
                ri, rv = ref
                live = rv > 0
                hit = (ri[:, :, None] == hi[:, None, :]).any(2) & live
                say("      recall@%d against similarityMH_knn (its %d entries with value > 0): %d = %.4f; rows with all of them found: %d of %d"
                    % (TOP, int(live.sum()), int(hit.sum()), hit.sum() / max(int(live.sum()), 1), int((hit.sum(1) == live.sum(1)).sum()), m))
                rec.update(recall_at_top=float(hit.sum() / max(int(live.sum()), 1)))
            result.append(rec)
            del hold
        del sig, ds
        torch.cuda.empty_cache()
        _capi.load().da_release_device_memory()
    if verdicts:
        worst = max(v[3] for v in verdicts)
        say("expectation %s: the stages after verify take %s of the kernel time of a device call (%s)"
            % ("CONFIRMED" if worst < 0.25 else "REFUTED", " / ".join("%.1f %%" % (100 * v[3]) for v in verdicts),
               ", ".join("%d %dx%d" % v[:3] for v in verdicts)))
    else:
        say("expectation: not measured (no kernel trace)")
    say("not measured: similarityMH_knn at the larger sizes (n^2 compares); counters; more than one device")
    say(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
