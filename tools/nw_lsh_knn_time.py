#!/usr/bin/env python3
"""Timing of the NW-ranked nearest-neighbour lists on MinHash LSH candidates on one MI355X (profiles/r27_a_nw_lsh_knn_timing.txt; DESIGN.md
section 7).

    python tools/nw_lsh_knn_time.py [--reps 5] [--short-n 100000] [--ha 4000,16000] [--no-trace] [--out FILE]
    python tools/nw_lsh_knn_time.py --kernels-only --set ha --n 4000
        (what the tool itself runs under `rocprofv3 --kernel-trace --output-format csv -d DIR --`, a process of its own, for the share of
        leg (a)'s kernel time that lies after the rescore)

k = 4, n_hash = 500, 100 bands x 5 rows, seed 12345, mh_threshold 0.5, NW threshold 0, top = 10, BLOSUM62 10 / 4.  Host clock around calls
that end in a device synchronise; per input one untimed warm-up round, then --reps rounds in which the legs ALTERNATE (a, b, c, a, ...);
medians.  Before any timing the lists of (a) and (b) are compared: indices equal, values equal as bit patterns.

  legs   a      similarityNW_lsh_knn on the strings (the new host entry)
         b      the only route to the same lists before it: similarityNW_lsh_edges(threshold=0) -> the whole candidate list on the host ->
                a numpy lexsort selection (both directions of every pair, value descending, column ascending, the first top of each row)
         c      similarityNW_knn_long at the first size of --ha: all pairs; other lists, so only its time is taken
  inputs synth.h3n2_like 20-mers made distinct (100 000 drawn, 44 931 distinct); synth.h3n2_like 566-mers (HA-like) at the sizes of --ha
         (3 rounds at the larger one).

EXPECTATION, written before the first run: (a) beats (b) by what (b) spends taking 12 bytes a candidate across the host boundary (plus the
8-byte weight it builds there) and sorting them in numpy: for the 20-mers, where 1.2e6 alignments take a few milliseconds, that is most of
(b) -- a lexsort of 2.4e6 entries alone is some hundred milliseconds -- so a large ratio, 5 x or more; for the HA-like sets, where 0.74 s /
11.9 s of alignments dominate, the boundary was 12 - 15 % of the edge call and the numpy sort of 8e6 / 1.3e8 entries comes on top, so (a)
wins 1.5 - 3 x there, more at 16 000 where the sort is 1.3e8 entries.  (c) at 4 000 HA-like sequences (1.18 s for the edge form) is slower
than (a) by about the 1.5 x of the r26 measurement.  The steps this pull request added -- rank keys, entries, selection -- are
bandwidth-bound passes over 4 .. 8 bytes a candidate: under 2 % of (a)'s kernel time where alignments dominate, 10 - 30 % for the 20-mers.
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, N_HASH, BANDS, ROWS, SEED, MH_THR, THR, TOP = 4, 500, 100, 5, 12345, 0.5, 0.0, 10


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"min": float(a[0]), "median": float(np.median(a)), "max": float(a[-1]), "reps": len(a)}


def fmt(s):
    return "min %10.3f  median %10.3f  max %10.3f ms  (%d reps)" % (s["min"], s["median"], s["max"], s["reps"])


def alternate(torch, legs, reps):
    """legs: {name: fn}; one warm-up round, then `reps` rounds a, b, ... -> {name: stats}"""
    out = {name: [] for name in legs}
    for r in range(1 + reps):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t) * 1e3
            if ms > 1000.0:                                   # a long run is not silent
                print("    round %d leg %s: %.0f ms" % (r, name, ms), file=sys.stderr, flush=True)
            if r:
                out[name].append(ms)
    return {name: stats(v) for name, v in out.items()}


def progress(lines, count):
    print("\n".join(lines[-count:]), file=sys.stderr, flush=True)


def distinct_strings(n, length):
    from dynaalign_amd import synth
    res, off = synth.h3n2_like(n, length)
    return list(dict.fromkeys(synth.to_strings(res, off)))


def new_route(da, seqs):
    return da.similarityNW_lsh_knn(seqs, K, N_HASH, BANDS, ROWS, TOP, mh_threshold=MH_THR, threshold=THR, seed=SEED)


def old_route(da, seqs):
    """the candidate list to the host, then the selection in numpy"""
    _, i, j, w = da.similarityNW_lsh_edges(seqs, K, N_HASH, BANDS, ROWS, THR, mh_threshold=MH_THR, seed=SEED)
    n = len(seqs)
    off = i != j
    i, j, w = i[off].astype(np.int64), j[off].astype(np.int64), w[off]
    r, c, v = np.concatenate([i, j]), np.concatenate([j, i]), np.concatenate([w, w])
    order = np.lexsort((c, -v, r))
    r, c, v = r[order], c[order], v[order]
    place = np.arange(len(r)) - np.searchsorted(r, np.arange(n))[r]
    keep = place < TOP
    idx = np.full((n, TOP), -1, np.int32)
    val = np.zeros((n, TOP), np.float64)
    idx[r[keep], place[keep]] = c[keep]
    val[r[keep], place[keep]] = v[keep]
    return idx, val


def case(torch, da, seqs, reps, lines, what, all_pairs):
    a, b = new_route(da, seqs), old_route(da, seqs)
    route = da.nw_lsh_last_route()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)), "the new entry and the old route disagree"
    new_route(da, seqs)
    route_a = da.nw_lsh_last_route()
    legs = {"a": lambda: new_route(da, seqs), "b": lambda: old_route(da, seqs)}
    if all_pairs:
        legs["c"] = lambda: da.similarityNW_knn_long(seqs, top=TOP)
    t = alternate(torch, legs, reps)
    lines.append("  %s, n = %d: %d candidates aligned (%d short, %d long); %d list entries of %d slots; lists of (a) and (b) equal bit for bit" %
                 (what, len(seqs), route["aligned_pairs"], route["short_pairs"], route["long_pairs"], route_a["edges"], len(seqs) * TOP))
    lines.append("      (a) similarityNW_lsh_knn                               %s" % fmt(t["a"]))
    lines.append("      (b) similarityNW_lsh_edges(threshold=0) + numpy lexsort %s" % fmt(t["b"]))
    lines.append("      (b) / (a) = %.2f" % (t["b"]["median"] / t["a"]["median"]))
    if all_pairs:
        lines.append("      (c) similarityNW_knn_long (all pairs)                   %s   (c) / (a) = %.2f" % (fmt(t["c"]), t["c"]["median"] / t["a"]["median"]))
    progress(lines, 5 if all_pairs else 4)
    return {"what": what, "n": len(seqs), "route": route_a, "ms": t}


def kernels_only(da, which, n):
    import torch
    seqs = distinct_strings(n, 20 if which == "short" else 566)
    new_route(da, seqs)
    torch.cuda.synchronize()
    new_route(da, seqs)                                       # the traced call: the last k_lsh_band_keys ... k_lsh_knn_select_long
    torch.cuda.synchronize()


def share_from_trace(trace_dir):
    """device time (ms) of the LAST host-entry call in a rocprofv3 kernel trace: every kernel behind the previous call's selection (the
    signatures and the encoding included), and what lies after the rescore -- from k_nwl_rank_keys on"""
    rows = []
    for f in sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)):
        for r in csv.DictReader(open(f)):
            k = {key.lower(): v for key, v in r.items()}
            rows.append((int(k["start_timestamp"]), int(k["end_timestamp"]), k["kernel_name"]))
    rows.sort()
    starts = [t for t, r in enumerate(rows) if "k_lsh_band_keys" in r[2]]
    if not starts:
        return None
    earlier = [t for t, r in enumerate(rows[:starts[-1]]) if "k_lsh_knn_select_long" in r[2]]
    rows = rows[earlier[-1] + 1 if earlier else 0:]
    total = after = 0.0
    behind = False
    by_kernel = {}
    for b, e, name in rows:
        behind = behind or "k_nwl_rank_keys" in name
        ms = (e - b) * 1e-6
        total += ms
        if behind:
            after += ms
            found = re.search(r"\bk_[a-z0-9_]+", name)
            short = found.group(0) if found else ("hipcub / rocprim" if "rocprim" in name or "hipcub" in name else name[:40])
            by_kernel[short] = by_kernel.get(short, 0.0) + ms
    return {"total_ms": total, "after_rescore_ms": after, "after_by_kernel_ms": by_kernel}


def trace_share(which, n):
    """one host-entry call under rocprofv3 --kernel-trace in a child process of its own"""
    d = tempfile.mkdtemp(prefix="nw_lsh_knn_trace_")
    try:
        print("tracing leg (a) on the %s set, n = %d ..." % (which, n), file=sys.stderr, flush=True)
        cmd = [shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--kernels-only", "--set", which, "--n", str(n)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        except subprocess.TimeoutExpired as e:
            # a traced child that hangs ends the tool: nothing more is started on the GPU
            raise SystemExit("the traced child (%s, n = %d) did not end within 300 s; nothing more is run\n%s"
                             % (which, n, (e.output or b"").decode("latin-1")[-4000:]))
        if p.returncode != 0:
            sys.stderr.write(p.stdout.decode("latin-1")[-4000:])
            raise SystemExit("the traced child (%s, n = %d) ended with status %d; nothing more is run" % (which, n, p.returncode))
        return share_from_trace(d)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--short-n", type=int, default=100000)
    ap.add_argument("--ha", default="4000,16000")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--set", default="ha", choices=("short", "ha"))
    ap.add_argument("--n", type=int, default=4000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import dynaalign_amd as da
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")
    if args.kernels_only:
        kernels_only(da, args.set, args.n)
        return
    lines = ["NW-ranked nearest-neighbour lists on MinHash LSH candidates; k = %d, n_hash = %d, %d x %d, seed %d, mh_threshold %.2f, threshold %.2f, "
             "top = %d, BLOSUM62 10 / 4; 1 warm-up round + %d rounds, legs alternated" % (K, N_HASH, BANDS, ROWS, SEED, MH_THR, THR, TOP, args.reps)]
    records = []
    seqs = distinct_strings(args.short_n, 20)
    lines.append("h3n2-like 20-mers: %d drawn, %d distinct" % (args.short_n, len(seqs)))
    records.append(case(torch, da, seqs, args.reps, lines, "20-mers", False))
    sizes = [int(v) for v in args.ha.split(",") if v]
    for pos, n in enumerate(sizes):
        seqs = distinct_strings(n, 566)
        lines.append("HA-like 566-mers: %d drawn, %d distinct" % (n, len(seqs)))
        records.append(case(torch, da, seqs, args.reps if pos == 0 else min(args.reps, 3), lines, "566-mers", pos == 0))
    if not args.no_trace:
        for which, n in (("short", args.short_n), ("ha", sizes[0] if sizes else 4000)):
            s = trace_share(which, n)
            if s is None:
                lines.append("  kernel trace of (a), %s set: no pipeline found in the trace" % which)
                continue
            lines.append("  kernel trace of one (a) call, %s set (n drawn = %d): %.3f ms of kernels, %.3f ms (%.2f %%) after the "
                         "rescore: %s" % (which, n, s["total_ms"], s["after_rescore_ms"], 100.0 * s["after_rescore_ms"] / max(s["total_ms"], 1e-9),
                                          ", ".join("%s %.3f" % kv for kv in sorted(s["after_by_kernel_ms"].items(), key=lambda kv: -kv[1]))))
            progress(lines, 1)
            records.append({"what": "trace", "set": which, "n": n, **s})
    lines.append("not measured: (c) at the sizes of --ha behind the first and on the 20-mers (similarityNW_knn_long on 44 931 20-mers is another problem "
                 "size: all pairs); the device route on resident data; more than one device")
    text = "\n".join(lines) + "\n" + json.dumps(records) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
