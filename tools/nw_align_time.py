#!/usr/bin/env python3
"""Timing of the alignment-path calls on one MI355X (profiles/r09_a_nw_align_timing.txt).

    python tools/nw_align_time.py [--reps 5] [--out FILE]       the timings
    python tools/nw_align_time.py --kernels-only                  three device calls per input, for a kernel trace
                                                                  (rocprofv3 --kernel-trace --stats -- python tools/nw_align_time.py --kernels-only)

Two inputs, BLOSUM62, gapOpen 10, gapExt 4, pairs drawn with a fixed seed (repeats allowed, no order):
  short  10^6 pairs among 100 000 h3n2-like 20-mers
  long   10^5 pairs among 20 000 uniform 127-mers
Host clock around calls that end in a device synchronise, 2 warm-up calls, --reps timed calls per leg, legs alternated in one process;
every leg is reported as min / median / max.

  a  host boundary: da_nw_align_pairs through ctypes on packed arrays (upload, kernels, results to the host), with and without ops;
     and nw_align(), which adds the Python strings
  b  device only: device.nw_align_pairs on resident codes and lists with a preallocated workspace, with and without ops
  c  the CPU oracle's orc_nw_pair, one thread, on the first --oracle-pairs pairs of the same lists (through ctypes, call overhead included)
  d  cells per second of (b) beside the direct sweep of similarityNW at N = 100 000 (402 ms for 5.00005e9 pairs of 400 cells, README):
     what a kernel that keeps no path reaches
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MATRIX, GO, GE = "BLOSUM62", 10, 4
SWEEP_MS, SWEEP_N, SWEEP_LEN = 402.0, 100000, 20      # the direct sweep of similarityNW (README)


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
    ap.add_argument("--oracle-pairs", type=int, default=20000)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import dynaalign_amd as da
    from dynaalign_amd import device, synth, _capi
    lib = _capi.load()
    if lib.da_device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured")
    rng = np.random.default_rng(20261017)
    inputs = {}
    res, off = synth.h3n2_like(100000, 20)
    inputs["short"] = (res, off, 20, rng.integers(0, 100000, 1000000).astype(np.int32), rng.integers(0, 100000, 1000000).astype(np.int32))
    res, off = synth.uniform_peptides(20000, 127, seed=9)
    inputs["long"] = (res, off, 127, rng.integers(0, 20000, 100000).astype(np.int32), rng.integers(0, 20000, 100000).astype(np.int32))
    lines, result = [], {}

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    if not a.kernels_only:
        say("alignment paths of listed pairs, %s, gapOpen %d, gapExt %d; 2 warm-up + %d timed calls per leg, legs alternated" % (MATRIX, GO, GE, a.reps))
    sweep_cells = SWEEP_N * (SWEEP_N + 1) / 2 * SWEEP_LEN * SWEEP_LEN / (SWEEP_MS * 1e-3)
    for name, (res, off, length, px, py) in inputs.items():
        pairs, ld = len(px), 2 * length
        ds = device.DeviceSequences(res, off)
        assert int(device.nw_encode(ds).item()) == 0
        tx, ty = torch.from_numpy(px).cuda(), torch.from_numpy(py).cuda()
        work = torch.empty(device.nw_align_workspace_bytes(min(pairs, 1 << 19)), dtype=torch.uint8, device="cuda")
        dev = lambda ops: device.nw_align_pairs(ds, ds, MATRIX, GO, GE, pair_x=tx, pair_y=ty, ops=ops, ld_ops=ld, work=work)   # noqa: E731
        if a.kernels_only:
            for _ in range(3):
                dev(True)
            torch.cuda.synchronize()
            continue
        ops_h = np.empty((pairs, ld), np.uint8)
        ln, mt, sc = (np.empty(pairs, np.int32) for _ in range(3))
        n = len(off) - 1

        def host(ops):
            _capi.check(lib.da_nw_align_pairs(res.ctypes.data, off.ctypes.data, n, res.ctypes.data, off.ctypes.data, n, px.ctypes.data, py.ctypes.data,
                                              pairs, MATRIX.encode(), GO, GE, ops_h.ctypes.data if ops else None, ld, ln.ctypes.data, mt.ctypes.data,
                                              sc.ctypes.data))
        seqs = synth.to_strings(res, off)
        legs = {"b  device, ops": lambda: dev(True), "b  device, no ops": lambda: dev(False),
                "a  da_nw_align_pairs, ops": lambda: host(True), "a  da_nw_align_pairs, no ops": lambda: host(False),
                "a  nw_align(), ops": lambda: da.nw_align(seqs, seqs, pairs=(px, py)),
                "a  nw_align(), no ops": lambda: da.nw_align(seqs, seqs, pairs=(px, py), ops=False)}
        r = alternate(torch, legs, a.reps)
        # the two boundaries agree
        d_ops, d_ln, d_mt, d_sc = dev(True)
        host(True)
        assert np.array_equal(d_ln.cpu().numpy(), ln) and np.array_equal(d_mt.cpu().numpy(), mt) and np.array_equal(d_ops.cpu().numpy(), ops_h)
        cells = pairs * length * length
        say("%s: %d pairs of %d-mers (%.3g cells, %.2f GB of decision words, ops rows of %d bytes)" % (name, pairs, length, cells, cells / 4 / 1e9, ld))
        for k_, v in r.items():
            say("     %-32s %s   %.3g pairs/s" % (k_, fmt(v), pairs / (v["median"] * 1e-3)))
        import oracle_lib as O
        k = min(a.oracle_pairs, pairs)
        t = time.perf_counter()
        for p in range(k):
            O.nw_pair(seqs[px[p]], seqs[py[p]], MATRIX, GO, GE)
        cpu_s = time.perf_counter() - t
        say("  c  orc_nw_pair, one thread, %d of these pairs through ctypes: %.1f ms -> %.3g pairs/s" % (k, cpu_s * 1e3, k / cpu_s))
        for leg in ("b  device, ops", "b  device, no ops"):
            rate = cells / (r[leg]["median"] * 1e-3)
            say("  d  %-20s %.3g cells/s = %.1f %% of the direct sweep of similarityNW (%.3g cells/s)" % (leg[3:], rate, 100 * rate / sweep_cells, sweep_cells))
        result[name] = {"pairs": pairs, "length": length, "legs": r, "oracle_pairs_per_s": k / cpu_s, "sweep_cells_per_s": sweep_cells}
        del work, tx, ty, ds
        torch.cuda.empty_cache()
        lib.da_release_device_memory()
    if a.kernels_only:
        return
    say(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
