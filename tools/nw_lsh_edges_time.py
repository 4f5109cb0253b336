#!/usr/bin/env python3
"""Timing of the NW identity on MinHash LSH candidates on one MI355X (profiles/r26_a_nw_lsh_edges_timing.txt).

    python tools/nw_lsh_edges_time.py [--reps 5] [--short-n 100000] [--ha 4000,16000] [--all-pairs-short 20000] [--out FILE]
    python tools/nw_lsh_edges_time.py --classes-only                                     the class question alone

k = 4, n_hash = 500, seed 12345, mh_threshold 0.5, NW threshold 0.5, BLOSUM62 10 / 4.  Host clock around calls that end in a device
synchronise; per input one untimed warm-up round, then --reps rounds in which the legs ALTERNATE (a, b, a, b, ...); medians.  Before any
timing the legs' lists are compared: indices equal, weights equal as bit patterns.

  legs   a      similarityNW_lsh_edges on the strings (the new host entry), and device.lsh_nw_edges on resident signatures + sequences
         b      the only route to the same list before it: similarityMH_lsh_edges -> the list on the host -> nw_align_long(pairs=, ops=False)
                -> matches / length and the threshold in numpy
         c      similarityNW_cross_edges[_long](x, x, threshold=): all pairs; its time and the recall of (a) against its upper triangle + diagonal
  inputs synth.h3n2_like 20-mers made distinct, 100 x 5 and 50 x 10 (c on the first --all-pairs-short strings only);
         synth.h3n2_like 566-mers (HA-like) at the sizes of --ha, 100 x 5 (c at the first size only);
         a mixed-length pair list for the class question of nw_lsh_kernels.hip: device.nw_rescore_pairs on random pairs of peptides of
         8 .. 127 residues in listed order against the same pairs ordered by the lane-per-pair kernel's strip class ceil(max(len) / 32)
         (sorted on the host, untimed: the most a finer partition on the device could win), and the same list with 1 % of pairs of
         300 .. 600 residues against da_dev_nw_align_long_pairs, which sends every pair through the wavefront kernel.

EXPECTATION, written before the first run: (a) beats (b) by at least what (b) spends moving the list across the host boundary twice and
running the host-side split -- for 20-mers, where the alignments take a few milliseconds, that is most of (b); for HA-like sequences the
alignments dominate both and the two come close.  (a) beats (c) by about the ratio of all pairs to candidates for the long sequences.
The strip-class order wins something on uniform lengths (a wave runs as long as its longest pair: with 64 uniform lengths per wave the
expected maximum is near 127, so up to ~2x in the fill kernel); whether that survives in whole-call time is what is measured.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, N_HASH, SEED, MH_THR, THR = 4, 500, 12345, 0.5, 0.5


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
            if r:
                out[name].append((time.perf_counter() - t) * 1e3)
    return {name: stats(v) for name, v in out.items()}


def progress(lines, count):
    """the lines a case just added, to stderr at once: a long run is not silent"""
    print("\n".join(lines[-count:]), file=sys.stderr, flush=True)


def distinct_strings(n, length):
    from dynaalign_amd import synth
    res, off = synth.h3n2_like(n, length)
    return list(dict.fromkeys(synth.to_strings(res, off)))


def same(a, b):
    return all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(a[:2], b[:2])) and \
        np.array_equal(np.asarray(a[2], np.float64).view(np.uint64), np.asarray(b[2], np.float64).view(np.uint64))


def old_route(da, seqs, bands, rows):
    _, i, j, _ = da.similarityMH_lsh_edges(seqs, K, N_HASH, bands, rows, MH_THR, seed=SEED)
    al = da.nw_align_long(seqs, seqs, pairs=(i, j), ops=False)
    w = al.matches.astype(np.float64) / al.length.astype(np.float64)
    keep = (w >= THR) & (w > 0)
    return i[keep], j[keep], w[keep]


def lsh_case(torch, da, device, seqs, bands, rows, reps, lines, what):
    new = lambda: da.similarityNW_lsh_edges(seqs, K, N_HASH, bands, rows, THR, mh_threshold=MH_THR, seed=SEED)[1:]   # noqa: E731
    a, b = new(), old_route(da, seqs, bands, rows)
    assert same(a, b), "the new entry and the old route disagree"
    route = da.nw_lsh_last_route()
    ds = device.DeviceSequences(*da.pack_sequences(seqs))
    device.nw_encode(ds)
    sig, _ = device.minhash_signatures(ds, K, N_HASH, da.hash_family_seeds(SEED, N_HASH), want_planes=False)
    cap = len(a[0])
    di, dj, dm, dl = device.lsh_nw_edges(sig, ds, N_HASH, bands, rows, THR, mh_threshold=MH_THR, capacity=cap)
    assert same(a, (di.cpu().numpy(), dj.cpu().numpy(), dm.cpu().numpy().astype(np.float64) / dl.cpu().numpy().astype(np.float64)))
    t = alternate(torch, {"a_host": new, "b_old": lambda: old_route(da, seqs, bands, rows),
                          "a_device": lambda: device.lsh_nw_edges(sig, ds, N_HASH, bands, rows, THR, mh_threshold=MH_THR, capacity=cap)}, reps)
    lines.append("  %s, %3d bands x %2d rows: %d candidates aligned (%d short, %d long), %d edges" %
                 (what, bands, rows, route["aligned_pairs"], route["short_pairs"], route["long_pairs"], route["edges"]))
    lines.append("      (a) similarityNW_lsh_edges, host boundary   %s" % fmt(t["a_host"]))
    lines.append("      (a) device.lsh_nw_edges, resident data      %s" % fmt(t["a_device"]))
    lines.append("      (b) MH lsh edges -> host -> nw_align_long   %s" % fmt(t["b_old"]))
    lines.append("      (b) / (a host) = %.2f" % (t["b_old"]["median"] / t["a_host"]["median"]))
    progress(lines, 5)
    return {"what": what, "n": len(seqs), "bands": bands, "rows": rows, "route": route, "ms": t}, a


def all_pairs(torch, da, seqs, long_, reps, lines, got, what):
    fn = da.similarityNW_cross_edges_long if long_ else da.similarityNW_cross_edges
    run = lambda: fn(seqs, seqs, threshold=THR)   # noqa: E731
    _, i, j, w = run()
    t = alternate(torch, {"c": run}, reps)["c"]
    upper = i <= j
    want = set(zip(i[upper].tolist(), j[upper].tolist()))
    have = set(zip(np.asarray(got[0]).tolist(), np.asarray(got[1]).tolist()))
    lines.append("      (c) all pairs, %s: %s; %d edges with i <= j; recall of (a) %d / %d = %.4f (%d edges of (a) are not in it)" %
                 (what, fmt(t), len(want), len(have & want), len(want), len(have & want) / max(len(want), 1), len(have - want)))
    progress(lines, 1)
    return {"what": what, "n": len(seqs), "all_pairs_ms": t, "all_pairs_edges": len(want), "recall": len(have & want) / max(len(want), 1)}


def class_question(torch, da, device, reps, lines):
    rng = np.random.RandomState(1)
    aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
    lens = np.r_[rng.randint(8, 128, 20000), rng.randint(300, 601, 200)]
    seqs = [aa[rng.randint(0, 20, n)].tobytes().decode() for n in lens]
    ds = device.DeviceSequences(*da.pack_sequences(seqs))
    device.nw_encode(ds)
    pairs = 2000000
    i, j = rng.randint(0, 20000, pairs).astype(np.int32), rng.randint(0, 20000, pairs).astype(np.int32)
    order = np.argsort((np.maximum(lens[i], lens[j]) + 31) // 32, kind="stable")
    mixed_i, mixed_j = i.copy(), j.copy()
    spots = rng.choice(pairs, pairs // 100, replace=False)
    mixed_i[spots] = rng.randint(20000, 20200, len(spots))
    mixed_j[spots] = rng.randint(20000, 20200, len(spots))
    dev = lambda a: torch.from_numpy(a).cuda()   # noqa: E731
    ti, tj, si, sj, mi, mj = dev(i), dev(j), dev(i[order]), dev(j[order]), dev(mixed_i), dev(mixed_j)
    work = torch.empty(device.nw_rescore_workspace_bytes(pairs), dtype=torch.uint8, device="cuda")
    listed = device.nw_rescore_pairs(ds, ds, ti, tj, work=work)
    by_class = device.nw_rescore_pairs(ds, ds, si, sj, work=work)
    assert all(np.array_equal(a.cpu().numpy()[order], b.cpu().numpy()) for a, b in zip(listed, by_class))
    new = device.nw_rescore_pairs(ds, ds, mi, mj, work=work)
    old = device.nw_align_long_pairs(ds, ds, pair_x=mi, pair_y=mj, ops=False, max_len=600)
    assert torch.equal(new[0], old[2]) and torch.equal(new[1], old[1])
    t = alternate(torch, {"listed": lambda: device.nw_rescore_pairs(ds, ds, ti, tj, work=work),
                          "by_class": lambda: device.nw_rescore_pairs(ds, ds, si, sj, work=work),
                          "mixed_new": lambda: device.nw_rescore_pairs(ds, ds, mi, mj, work=work),
                          "mixed_all_long": lambda: device.nw_align_long_pairs(ds, ds, pair_x=mi, pair_y=mj, ops=False, max_len=600)}, reps)
    lines.append("  class question: device.nw_rescore_pairs on %d random pairs of peptides of 8 .. 127 residues (uniform)" % pairs)
    lines.append("      listed order                                %s" % fmt(t["listed"]))
    lines.append("      ordered by strip class ceil(max(len) / 32)  %s   listed / ordered = %.2f" %
                 (fmt(t["by_class"]), t["listed"]["median"] / t["by_class"]["median"]))
    lines.append("  the same list with 1 % of pairs of 300 .. 600 residues:")
    lines.append("      device.nw_rescore_pairs (split on device)   %s" % fmt(t["mixed_new"]))
    lines.append("      device.nw_align_long_pairs (all wavefront)  %s   all wavefront / split = %.2f" %
                 (fmt(t["mixed_all_long"]), t["mixed_all_long"]["median"] / t["mixed_new"]["median"]))
    progress(lines, 6)
    return {"what": "class question", "pairs": pairs, "ms": t}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--short-n", type=int, default=100000)
    ap.add_argument("--ha", default="4000,16000")
    ap.add_argument("--all-pairs-short", type=int, default=20000)
    ap.add_argument("--classes-only", action="store_true", help="the class question alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import dynaalign_amd as da
    from dynaalign_amd import device
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")
    lines = ["NW identity on MinHash LSH candidates; k = %d, n_hash = %d, seed %d, mh_threshold %.2f, threshold %.2f, BLOSUM62 10 / 4; "
             "1 warm-up round + %d rounds, legs alternated" % (K, N_HASH, SEED, MH_THR, THR, args.reps)]
    records = []
    if args.classes_only:
        records.append(class_question(torch, da, device, args.reps, lines))
        sys.stdout.write("\n".join(lines) + "\n" + json.dumps(records) + "\n")
        return
    seqs = distinct_strings(args.short_n, 20)
    lines.append("h3n2-like 20-mers: %d drawn, %d distinct" % (args.short_n, len(seqs)))
    for bands, rows in ((100, 5), (50, 10)):
        rec, got = lsh_case(torch, da, device, seqs, bands, rows, args.reps, lines, "20-mers")
        records.append(rec)
    sub = seqs[:args.all_pairs_short]
    got = da.similarityNW_lsh_edges(sub, K, N_HASH, 100, 5, THR, mh_threshold=MH_THR, seed=SEED)[1:]
    records.append(all_pairs(torch, da, sub, False, args.reps, lines, got, "the first %d 20-mers, (a) at 100 x 5 on the same strings" % len(sub)))
    for idx, n in enumerate(int(v) for v in args.ha.split(",") if v):
        seqs = distinct_strings(n, 566)
        lines.append("HA-like 566-mers: %d drawn, %d distinct" % (n, len(seqs)))
        rec, got = lsh_case(torch, da, device, seqs, 100, 5, args.reps if idx == 0 else min(args.reps, 3), lines, "566-mers")
        records.append(rec)
        if idx == 0:
            records.append(all_pairs(torch, da, seqs, True, min(args.reps, 3), lines, got, "%d 566-mers" % len(seqs)))
    records.append(class_question(torch, da, device, args.reps, lines))
    lines.append("not measured: (c) at the larger sizes; the largest n at which (b) still finishes (the larger --ha size is only the largest one "
                 "run); kernel traces and counters; more than one device")
    text = "\n".join(lines) + "\n" + json.dumps(records) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
