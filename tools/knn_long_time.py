#!/usr/bin/env python3
"""Timing of the long NW nearest-neighbour lists on one MI355X (profiles/r15_a_knn_long_timing.txt).

    python tools/knn_long_time.py [--n 4000] [--reps 3] [--out FILE]            the timings
    python tools/knn_long_time.py --kernels-only                                 two warm-up calls + one traced call of (a), for a kernel trace
        (rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/knn_long_time.py --kernels-only)
    python tools/knn_long_time.py --summarise-trace DIR [--call-ms MS]           per-kernel totals of that trace and their share of a call

BLOSUM62, gapOpen 10, gapExt 4, top 10.  Input: synth.h3n2_like(n, 566), n chosen so that the n x n block of 4-byte keys fits one block
(the one-set form then runs the symmetric sweep).  Host clock around calls that end in a device synchronise, 2 warm-up calls, --reps timed
calls per leg, legs alternated in one process; every leg is reported as min / median / max.

  a  similarityNW_knn_long(seqs, top=10) at the host boundary: upload, DP, ranks, the selection, the lists to the host
  b  the yardstick it replaces: similarityNW(seqs) (the dense float64 n x n matrix to the host) + knn_dense on it
  c  da_dev_nw with DA_OUT_PACK32 alone on the resident codes (symmetric sweep): the floor (a) cannot beat
  d  (a) again with DYNAALIGN_BLOCK_BYTES set so that the square is cut into two row blocks: every pair is computed twice

Expectations to confirm or refute: a = c + upload; d = 2 x the DP.
"""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MATRIX, GO, GE, TOP, LEN_HA = "BLOSUM62", 10, 4, 10, 566
NEW_KERNELS = ("k_codes_to_ranks", "k_topk_ranks")


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"min": float(a[0]), "median": float(np.median(a)), "max": float(a[-1]), "reps": len(a)}


def fmt(s):
    return "min %10.3f  median %10.3f  max %10.3f ms  (%d reps)" % (s["min"], s["median"], s["max"], s["reps"])


def summarise(trace_dir, call_ms, say):
    """kernel totals of the LAST traced call (every call starts with k_nw_encode)"""
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % trace_dir)
    rows = []
    for f in files:
        for r in csv.DictReader(open(f)):
            k = {key.lower(): v for key, v in r.items()}
            rows.append((int(k["start_timestamp"]), int(k["end_timestamp"]), k["kernel_name"]))
    rows.sort()
    starts = [t for t, (_, _, name) in enumerate(rows) if "k_nw_encode" in name]
    rows = rows[starts[-1]:] if starts else rows
    total = {}
    for b, e, name in rows:
        short = name.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").replace("da::", "")
        c, ms = total.get(short, (0, 0.0))
        total[short] = (c + 1, ms + (e - b) * 1e-6)
    all_ms = sum(ms for _, ms in total.values())
    say("kernels of one similarityNW_knn_long call (rocprofv3 --kernel-trace, a run of its own), device time %.3f ms%s"
        % (all_ms, "" if call_ms is None else "; share of the call's %.1f ms at the host boundary" % call_ms))
    say("%-44s %6s %12s %9s" % ("kernel", "calls", "ms", "share"))
    for name, (c, ms) in sorted(total.items(), key=lambda kv: -kv[1][1]):
        say("%-44s %6d %12.3f %8.3f%%" % (name[:44], c, ms, 100 * ms / (call_ms if call_ms else all_ms)))
    new_ms = sum(ms for name, (_, ms) in total.items() if any(k in name for k in NEW_KERNELS))
    say("the ranks and the selection together: %.3f ms = %.3f %% of %s" % (new_ms, 100 * new_ms / (call_ms if call_ms else all_ms),
                                                                           "the call" if call_ms else "the device time"))


class block_bytes:
    """DYNAALIGN_BLOCK_BYTES for the duration of a call (the Python mirror reloads the library's configuration when it changes)"""

    def __init__(self, value):
        self.value = str(int(value))

    def __enter__(self):
        self.old = os.environ.get("DYNAALIGN_BLOCK_BYTES")
        os.environ["DYNAALIGN_BLOCK_BYTES"] = self.value

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("DYNAALIGN_BLOCK_BYTES", None)
        else:
            os.environ["DYNAALIGN_BLOCK_BYTES"] = self.old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--summarise-trace", default=None)
    ap.add_argument("--call-ms", type=float, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def finish():
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
    if a.summarise_trace:
        summarise(a.summarise_trace, a.call_ms, say)
        return finish()
    import torch
    import dynaalign_amd as da
    from dynaalign_amd import _capi, device, synth
    if _capi.load().da_device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured")
    n = a.n
    res, off = synth.h3n2_like(n, LEN_HA)
    seqs = synth.to_strings(res, off)
    lists = lambda: da.similarityNW_knn_long(seqs, MATRIX, GO, GE, TOP)   # noqa: E731
    if a.kernels_only:
        for _ in range(3):
            lists()
        torch.cuda.synchronize()
        return
    ds = device.DeviceSequences(res, off)
    assert int(device.nw_encode(ds).item()) == 0
    codes = torch.empty((n, n), dtype=torch.int32, device="cuda")
    sweep = lambda: device.nw(ds, MATRIX, GO, GE, kind=_capi.DA_OUT_PACK32, out=codes)   # noqa: E731
    dense = lambda: da.knn_dense(da.similarityNW(seqs, MATRIX, GO, GE), TOP)              # noqa: E731
    ld = (n + 3) // 4 * 4
    half = ((n // 2 + 7) // 8 * 8) * ld * 4                                # the bytes of half the rows, to a multiple of 8: two blocks

    def two_blocks():
        with block_bytes(half):
            return lists()
    legs = {"a  similarityNW_knn_long": lists, "b  similarityNW + knn_dense": dense, "c  da_dev_nw, PACK32, resident": sweep,
            "d  similarityNW_knn_long, two row blocks": two_blocks}
    out = {k: [] for k in legs}
    keep = {}
    warm = 2
    for r in range(warm + a.reps):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            keep[name] = fn()
            torch.cuda.synchronize()
            if r >= warm:
                out[name].append((time.perf_counter() - t) * 1e3)
    r = {k: stats(v) for k, v in out.items()}
    names = list(legs)
    got, want, cut = keep[names[0]], keep[names[1]], keep[names[3]]
    for g in (got, cut):
        assert np.array_equal(g[0], want[0]) and np.array_equal(g[1].view(np.uint64), want[1].view(np.uint64))
    pairs = n * (n - 1) // 2
    say("NW nearest-neighbour lists of sequences up to 1024 residues, %s, gapOpen %d, gapExt %d, top %d; %d warm-up + %d timed calls per leg, legs alternated"
        % (MATRIX, GO, GE, TOP, warm, a.reps))
    say("input: synth.h3n2_like(%d, %d): %d pairs, %.3g cells; (a), (b) and (d) agree bit for bit" % (n, LEN_HA, pairs, pairs * LEN_HA * LEN_HA))
    for k_, v in r.items():
        say("  %-42s %s" % (k_, fmt(v)))
    am, bm, cm, dm = (r[k_]["median"] for k_ in legs)
    say("  c in cells per second (triangle with the diagonal): %.3g" % ((pairs + n) * LEN_HA * LEN_HA / (cm * 1e-3)))
    say("  a - c = %.1f ms = %.1f %% of c: upload, table, the ranks, the selection, the lists to the host" % (am - cm, 100 * (am - cm) / cm))
    say("  d / c = %.2f, d / a = %.2f: the square in two row blocks computes every pair twice" % (dm / cm, dm / am))
    say("  b / a = %.2f" % (bm / am))
    finish()


if __name__ == "__main__":
    main()
