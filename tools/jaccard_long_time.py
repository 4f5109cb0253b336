#!/usr/bin/env python3
"""Timing of the exact Jaccard index for sequences of up to 1024 shingles on one MI355X (profiles/r19_a_jaccard_long_timing.txt; DESIGN.md
section 7).

    python tools/jaccard_long_time.py [--n 4000] [--reps 3] [--out FILE]         the timings
    python tools/jaccard_long_time.py --kernels-only                              two warm-up calls + one more call of (a), for a kernel trace
        (rocprofv3 --kernel-trace --stats -d DIR -- python tools/jaccard_long_time.py --kernels-only: a run of its own)

k = 4, top 10.  Input: synth.h3n2_like(n, 566).  Host clock around calls that end in a device synchronise, 2 warm-up calls, --reps timed
calls per leg, legs alternated in one process; every leg is reported as min / median / max.

  a   device.jaccard_sets_long + device.jaccard_rect_long, the full square as PACK32 codes (a': the sets alone)
  b   device.minhash_signatures + device.mh_planes + device.mh_compare(kind = COMPACT) at n_hash = 50 and 500 on the same sequences: the
      estimate the exact index is an alternative to
  c   da_dev_nw with DA_OUT_PACK32 on the same sequences (symmetric sweep): the other exact long similarity
  d   similarityJaccard_knn_long(top = 10) at the host boundary, against d' similarityJaccard_long + knn_dense
  e   (d) again with DYNAALIGN_BLOCK_BYTES set so that the square is cut into two row blocks: full rows, every pair computed twice

Expectations to confirm or refute: a far below c; d about a plus the upload and the lists; e about d plus one more rectangle.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, TOP, LEN_HA, SEED = 4, 10, 566, 12345
MATRIX, GO, GE = "BLOSUM62", 10, 4


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"min": float(a[0]), "median": float(np.median(a)), "max": float(a[-1]), "reps": len(a)}


def fmt(s):
    return "min %10.3f  median %10.3f  max %10.3f ms  (%d reps)" % (s["min"], s["median"], s["max"], s["reps"])


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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    import torch
    import dynaalign_amd as da
    from dynaalign_amd import _capi, device, synth
    from dynaalign_amd._capi import DA_OUT_COMPACT, DA_OUT_PACK32
    if _capi.load().da_device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured")
    n = a.n
    res, off = synth.h3n2_like(n, LEN_HA)
    seqs = synth.to_strings(res, off)
    ds = device.DeviceSequences(res, off)
    codes = torch.empty((n, n), dtype=torch.int32, device="cuda")        # one result buffer for the 32-bit device legs
    counts = torch.empty((n, n), dtype=torch.int16, device="cuda")

    def exact():
        return device.jaccard_rect_long(device.jaccard_sets_long(ds, K), kind=DA_OUT_PACK32, out=codes)
    if a.kernels_only:
        for _ in range(3):
            exact()
        torch.cuda.synchronize()
        return
    seeds = {nh: da.hash_family_seeds(SEED, nh) for nh in (50, 500)}
    assert int(device.nw_encode(ds).item()) == 0

    def minhash(nh):
        sig, _ = device.minhash_signatures(ds, K, nh, seeds[nh], want_planes=False)
        return device.mh_compare(device.mh_planes(sig, n, nh), n, nh, kind=DA_OUT_COMPACT, out=counts)
    lists = lambda: da.similarityJaccard_knn_long(seqs, K, TOP)                             # noqa: E731
    ld = (n + 3) // 4 * 4
    half = ((n // 2 + 7) // 8 * 8) * ld * 4                                # the bytes of half the rows, to a multiple of 8: two blocks

    def two_blocks():
        with block_bytes(half):
            return lists()
    legs = {"a  jaccard_sets_long + jaccard_rect_long, PACK32": exact,
            "a' jaccard_sets_long alone": lambda: device.jaccard_sets_long(ds, K),
            "b  signatures + planes + mh_compare, n_hash = 50": lambda: minhash(50),
            "b  signatures + planes + mh_compare, n_hash = 500": lambda: minhash(500),
            "c  da_dev_nw, PACK32, resident": lambda: device.nw(ds, MATRIX, GO, GE, kind=DA_OUT_PACK32, out=codes),
            "d  similarityJaccard_knn_long": lists,
            "d' similarityJaccard_long + knn_dense": lambda: da.knn_dense(da.similarityJaccard_long(seqs, K), TOP),
            "e  similarityJaccard_knn_long, two row blocks": two_blocks}
    out = {name: [] for name in legs}
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
    r = {name: stats(v) for name, v in out.items()}
    names = list(legs)
    got, want, cut = keep[names[5]], keep[names[6]], keep[names[7]]
    for g in (got, cut):
        assert np.array_equal(g[0], want[0]) and np.array_equal(g[1].view(np.uint64), want[1].view(np.uint64))
    sets = device.jaccard_sets_long(ds, K)
    torch.cuda.synchronize()
    cnt = sets.counts.cpu().numpy().view(np.uint16)[:n].astype(np.int64)
    pairs = n * (n - 1) // 2
    say("exact Jaccard index of sequences up to 1024 shingles, k = %d, top %d; %d warm-up + %d timed calls per leg, legs alternated" % (K, TOP, warm, a.reps))
    say("input: synth.h3n2_like(%d, %d): %d pairs, %d .. %d distinct shingles a sequence (mean %.1f), ld_keys %d; (d), (d') and (e) agree bit for bit"
        % (n, LEN_HA, pairs, cnt.min(), cnt.max(), cnt.mean(), sets.ld_keys))
    for name, v in r.items():
        say("  %-52s %s" % (name, fmt(v)))
    am, cm, dm, em = r[names[0]]["median"], r[names[4]]["median"], r[names[5]]["median"], r[names[7]]["median"]
    say("  a in pairs per second (triangle with the diagonal): %.3g" % ((pairs + n) / (am * 1e-3)))
    say("  c / a = %.1f: the NW identity of the same sequences against their exact Jaccard index" % (cm / am))
    say("  a / b(50) = %.2f, a / b(500) = %.2f: the exact index against its MinHash estimate" % (am / r[names[2]]["median"], am / r[names[3]]["median"]))
    say("  d - a = %.1f ms: upload, table, the ranks, the selection, the lists to the host" % (dm - am))
    say("  e - d = %.1f ms, (e - d) / a = %.2f: the square in two row blocks computes full rows, every pair twice" % (em - dm, (em - dm) / am))
    say("  d' / d = %.2f" % (r[names[6]]["median"] / dm))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
