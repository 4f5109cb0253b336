#!/usr/bin/env python3
"""Timing of the long alignment-path calls on one MI355X (profiles/r10_a_nw_align_long_timing.txt).

    python tools/nw_align_long_time.py [--reps 5] [--out FILE]       the timings
    python tools/nw_align_long_time.py --kernels-only                  three device calls per leg, for a kernel trace
                                                                       (rocprofv3 --kernel-trace --stats -- python tools/nw_align_long_time.py --kernels-only)

BLOSUM62, gapOpen 10, gapExt 4.  The HA input: 10^4 listed pairs (fixed seed, repeats allowed, no order) among 2 000
synth.h3n2_like(2000, 566) sequences.  Host clock around calls that end in a device synchronise, 2 warm-up calls, --reps timed calls per
leg, legs alternated in one process; every leg is reported as min / median / max.

  a  host boundary: da_nw_align_long_pairs through ctypes on packed arrays (upload, kernel, results to the host), with and without ops;
     and nw_align_long(), which adds the Python strings
  b  device only: device.nw_align_long_pairs on resident codes and lists with a preallocated workspace, with and without ops.  The kernel
     is fused: there is no separate walk time, the difference of the two legs is the decision stores plus the walk
  c  the CPU oracle's orc_nw_pair, one thread, on the first --oracle-pairs pairs of the same list (through ctypes, call overhead included)
  d  the yardstick, same run, same box: the forward sweep da_dev_nw (k_nw_long) over the same 2 000 sequences in cells per second, and
     the no-ops leg of (b), which runs the same cell, beside it as a ratio.  10^4 pairs are 2.4 pairs per resident wave (3.3 per slot
     with ops), so the last round of the persistent grid runs part empty: the legs "full rounds" take 10 pairs per wave (per slot)
  e  a mixed list through the host call: 10^6 pairs of 20-mers plus 10^3 pairs of 566-mers in one da_nw_align_long_pairs call, beside
     the two parts on their own (the short part through da_nw_align_pairs): the cost of the split
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
N_HA, LEN_HA, PAIRS_HA = 2000, 566, 10000


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
    ap.add_argument("--oracle-pairs", type=int, default=200)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import dynaalign_amd as da
    from dynaalign_amd import device, synth, _capi
    lib = _capi.load()
    if lib.da_device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured")
    rng = np.random.default_rng(20261018)
    lines, result = [], {}

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    res, off = synth.h3n2_like(N_HA, LEN_HA)
    px, py = rng.integers(0, N_HA, PAIRS_HA).astype(np.int32), rng.integers(0, N_HA, PAIRS_HA).astype(np.int32)
    pairs, ld = PAIRS_HA, 2 * LEN_HA
    ds = device.DeviceSequences(res, off)
    assert int(device.nw_encode(ds).item()) == 0
    tx, ty = torch.from_numpy(px).cuda(), torch.from_numpy(py).cuda()
    wbytes = device.nw_align_long_workspace_bytes(pairs, LEN_HA)
    work = torch.empty(wbytes, dtype=torch.uint8, device="cuda")
    dev = lambda ops: device.nw_align_long_pairs(ds, ds, MATRIX, GO, GE, pair_x=tx, pair_y=ty, ops=ops, ld_ops=ld, max_len=LEN_HA, work=work)   # noqa: E731
    sweep_out = torch.empty((N_HA, N_HA), dtype=torch.float64, device="cuda")
    sweep = lambda: device.nw(ds, MATRIX, GO, GE, out=sweep_out)   # noqa: E731
    # full rounds of the persistent grid: 10 pairs for every wave without ops (4096 waves), 10 for every slot with ops
    slots = wbytes // device.nw_align_long_workspace_bytes(1, LEN_HA)
    full = {False: 40960, True: 10 * slots}
    fx = {k: torch.from_numpy(rng.integers(0, N_HA, v).astype(np.int32)).cuda() for k, v in full.items()}
    fy = {k: torch.from_numpy(rng.integers(0, N_HA, v).astype(np.int32)).cuda() for k, v in full.items()}
    dev_full = lambda ops: device.nw_align_long_pairs(ds, ds, MATRIX, GO, GE, pair_x=fx[ops], pair_y=fy[ops], ops=ops, ld_ops=ld, max_len=LEN_HA,   # noqa: E731
                                                      work=work)
    if a.kernels_only:
        for _ in range(3):
            dev(True)
            dev(False)
            dev_full(True)
            dev_full(False)
            sweep()
        torch.cuda.synchronize()
        return
    say("alignment paths of listed pairs of up to 1024 residues, %s, gapOpen %d, gapExt %d; 2 warm-up + %d timed calls per leg, legs alternated"
        % (MATRIX, GO, GE, a.reps))
    ops_h = np.empty((pairs, ld), np.uint8)
    ln, mt, sc = (np.empty(pairs, np.int32) for _ in range(3))

    def host(ops):
        _capi.check(lib.da_nw_align_long_pairs(res.ctypes.data, off.ctypes.data, N_HA, res.ctypes.data, off.ctypes.data, N_HA, px.ctypes.data,
                                               py.ctypes.data, pairs, MATRIX.encode(), GO, GE, ops_h.ctypes.data if ops else None, ld, ln.ctypes.data,
                                               mt.ctypes.data, sc.ctypes.data))
    seqs = synth.to_strings(res, off)
    legs = {"b  device, ops": lambda: dev(True), "b  device, no ops": lambda: dev(False), "d  da_dev_nw forward sweep": sweep,
            "d  full rounds, ops": lambda: dev_full(True), "d  full rounds, no ops": lambda: dev_full(False),
            "a  da_nw_align_long_pairs, ops": lambda: host(True), "a  da_nw_align_long_pairs, no ops": lambda: host(False),
            "a  nw_align_long(), ops": lambda: da.nw_align_long(seqs, seqs, pairs=(px, py)),
            "a  nw_align_long(), no ops": lambda: da.nw_align_long(seqs, seqs, pairs=(px, py), ops=False)}
    r = alternate(torch, legs, a.reps)
    # the two boundaries agree, and the no-ops leg gives the integers of the ops leg
    d_ops, d_ln, d_mt, d_sc = dev(True)
    n_ops = dev(False)
    host(True)
    assert np.array_equal(d_ln.cpu().numpy(), ln) and np.array_equal(d_mt.cpu().numpy(), mt) and np.array_equal(d_ops.cpu().numpy(), ops_h)
    assert np.array_equal(n_ops[1].cpu().numpy(), ln) and np.array_equal(n_ops[2].cpu().numpy(), mt) and np.array_equal(n_ops[3].cpu().numpy(), sc)
    cells = pairs * LEN_HA * LEN_HA
    say("HA: %d pairs among %d %d-mers (%.3g cells, %.2f GB of decision words through %d slots = %.0f MB of workspace, ops rows of %d bytes)"
        % (pairs, N_HA, LEN_HA, cells, pairs * (LEN_HA + 63) * 256 / 1e9, wbytes // device.nw_align_long_workspace_bytes(1, LEN_HA), wbytes / 1e6, ld))
    for k_, v in r.items():
        if k_[0] != "d":
            say("     %-36s %s   %.3g pairs/s" % (k_, fmt(v), pairs / (v["median"] * 1e-3)))
    diff = r["b  device, ops"]["median"] - r["b  device, no ops"]["median"]
    say("  b  decision stores + walk (ops leg minus no-ops leg, medians): %.3f ms = %.0f %% of the ops leg" % (diff, 100 * diff / r["b  device, ops"]["median"]))
    import oracle_lib as O
    k = min(a.oracle_pairs, pairs)
    t = time.perf_counter()
    for p in range(k):
        O.nw_pair(seqs[px[p]], seqs[py[p]], MATRIX, GO, GE)
    cpu_s = time.perf_counter() - t
    say("  c  orc_nw_pair, one thread, %d of these pairs through ctypes: %.1f ms -> %.3g pairs/s, %.3g cells/s"
        % (k, cpu_s * 1e3, k / cpu_s, k * LEN_HA * LEN_HA / cpu_s))
    sweep_cells = N_HA * (N_HA + 1) / 2 * LEN_HA * LEN_HA
    sweep_rate = sweep_cells / (r["d  da_dev_nw forward sweep"]["median"] * 1e-3)
    say("  d  da_dev_nw forward sweep, %d sequences (%.3g cells): %s -> %.3g cells/s" % (N_HA, sweep_cells, fmt(r["d  da_dev_nw forward sweep"]), sweep_rate))
    for leg in ("b  device, no ops", "b  device, ops"):
        rate = cells / (r[leg]["median"] * 1e-3)
        say("  d  %-20s %.3g cells/s = %.1f %% of the forward sweep" % (leg[3:], rate, 100 * rate / sweep_rate))
    for ops in (False, True):
        leg = "d  full rounds, %s" % ("ops" if ops else "no ops")
        rate = full[ops] * LEN_HA * LEN_HA / (r[leg]["median"] * 1e-3)
        say("  d  %-20s %d pairs: %s -> %.3g cells/s = %.1f %% of the forward sweep" % (leg[3:], full[ops], fmt(r[leg]), rate, 100 * rate / sweep_rate))
    result["ha"] = {"pairs": pairs, "length": LEN_HA, "legs": r, "oracle_pairs_per_s": k / cpu_s, "sweep_cells_per_s": sweep_rate}
    del work, tx, ty, fx, fy, sweep_out, ops_h
    torch.cuda.empty_cache()
    lib.da_release_device_memory()

    # e: the mixed list
    n_short, p_short, p_long = 100000, 1000000, 1000
    sres, soff = synth.h3n2_like(n_short, 20)
    mres = np.concatenate([sres, res])
    moff = np.concatenate([soff, off[1:] + soff[-1]])
    n_all = n_short + N_HA
    sx, sy = rng.integers(0, n_short, p_short).astype(np.int32), rng.integers(0, n_short, p_short).astype(np.int32)
    lx, ly = px[:p_long] + n_short, py[:p_long] + n_short
    at = rng.permutation(p_short + p_long)                     # the long pairs scattered among the short ones
    mx, my = np.concatenate([sx, lx])[at], np.concatenate([sy, ly])[at]

    def call(entry, qx, qy, ld_, ops_buf, ops):
        cnt = len(qx)
        o = [np.empty(cnt, np.int32) for _ in range(3)]
        _capi.check(getattr(lib, entry)(mres.ctypes.data, moff.ctypes.data, n_all, mres.ctypes.data, moff.ctypes.data, n_all, qx.ctypes.data,
                                        qy.ctypes.data, cnt, MATRIX.encode(), GO, GE, ops_buf.ctypes.data if ops else None, ld_, o[0].ctypes.data,
                                        o[1].ctypes.data, o[2].ctypes.data))
        return o
    big = np.empty((p_short + p_long, ld), np.uint8)
    small = np.empty((p_short, 40), np.uint8)
    legs = {"e  mixed list, one call, no ops": lambda: call("da_nw_align_long_pairs", mx, my, ld, big, False),
            "e  short part alone (da_nw_align_pairs), no ops": lambda: call("da_nw_align_pairs", sx, sy, 40, small, False),
            "e  long part alone, no ops": lambda: call("da_nw_align_long_pairs", lx, ly, ld, big, False),
            "e  mixed list, one call, ops": lambda: call("da_nw_align_long_pairs", mx, my, ld, big, True),
            "e  short part alone (da_nw_align_pairs), ops": lambda: call("da_nw_align_pairs", sx, sy, 40, small, True),
            "e  long part alone, ops": lambda: call("da_nw_align_long_pairs", lx, ly, ld, big, True)}
    r = alternate(torch, legs, max(a.reps // 2, 2), warm=1)
    say("mixed: %d pairs of 20-mers and %d pairs of %d-mers in one list (ops rows of %d bytes for every pair: %.2f GB to the host)"
        % (p_short, p_long, LEN_HA, ld, (p_short + p_long) * ld / 1e9))
    for k_, v in r.items():
        say("     %-50s %s" % (k_, fmt(v)))
    for kind in ("no ops", "ops"):
        whole = r["e  mixed list, one call, %s" % kind]["median"]
        parts = r["e  short part alone (da_nw_align_pairs), %s" % kind]["median"] + r["e  long part alone, %s" % kind]["median"]
        say("  e  %-6s one call %.1f ms, the two parts on their own %.1f ms: the split costs %+.1f ms" % (kind, whole, parts, whole - parts))
    result["mixed"] = {"short_pairs": p_short, "long_pairs": p_long, "legs": r}
    say(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
