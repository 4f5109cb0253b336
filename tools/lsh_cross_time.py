#!/usr/bin/env python3
"""Timing of the two-set LSH form on one MI355X (profiles/r22_a_lsh_cross_timing.txt).

    python tools/lsh_cross_time.py [--reps 5] [--sizes 100000,1000000] [--queries 4096] [--baseline-max 1000000] [--out FILE]

Input: a resident set synth.h3n2_like(n, 20) and a query batch synth.h3n2_like(queries, 20, seed_samples=29), each made distinct (first
occurrences, in order); k = 4, n_hash = 500, seed 12345, top = 10, threshold 0.5, bands x rows of 100 x 5 and 50 x 10.  Host clock around
calls that end in a device synchronise.  The legs of one (size, banding) are timed in ONE run and ALTERNATED -- round r runs every leg
once, in order -- after one warm-up round; min / median / max over --reps rounds.

  per size and banding:
    index build          device.lsh_index_build on the resident signatures, into a buffer that exists: keys, sort, tables
    topk / edges query   MinHashSession.lsh_cross_topk / lsh_cross_edges of the batch against the KEPT index: K1 on the query strings, probe,
                         verify, lists / edge list (the index is built before the first timed round and never again)
    topk / edges host    similarityMH_lsh_cross_topk / _edges on the strings of both sets: upload, both signature sets, the index, one query
    counts               runs of the index, (pair, band) incidences, distinct verified pairs, list entries / edges
  for resident sets of up to --baseline-max drawn sequences, in the same run: MinHashSession.cross_topk / cross_edges(threshold=) on the same
  inputs -- the rectangle compare, the existing code and the baseline -- and the recall of the LSH results against them (top-k: its entries
  with value > 0; edges: its edges).

EXPECTATION, written down before the first measurement: a query batch against a kept index costs less than the rectangle compare of the same
shape -- lsh_cross_topk under cross_topk and lsh_cross_edges under cross_edges(threshold=), medians of the same run, at every measured
(size, banding).  The tool prints the pairs and whether that held.  No speed figure is a pass condition of anything.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, N_HASH, SEED, TOP, THRESHOLD = 4, 500, 12345, 10, 0.5
BANDINGS = ((100, 5), (50, 10))


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


def distinct_strings(n, **kw):
    from dynaalign_amd import synth
    res, off = synth.h3n2_like(n, 20, **kw)
    return list(dict.fromkeys(synth.to_strings(res, off)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--baseline-max", type=int, default=1000000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import dynaalign_amd as da
    from dynaalign_amd import device, session, similarity, _capi
    if _capi.load().da_device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured")
    lines, result, verdicts = [], [], []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    new = distinct_strings(a.queries, seed_samples=29)
    say("two-set LSH, h3n2-like 20-mers made distinct, k = %d, n_hash = %d, seed %d, top = %d, threshold %.2f; %d query sequences (%d drawn); "
        "legs alternated, 1 warm-up + %d timed rounds" % (K, N_HASH, SEED, TOP, THRESHOLD, len(new), a.queries, a.reps))
    say("expectation (stated before measuring): a query batch against a kept index costs less than the rectangle compare of the same shape")
    for n in (int(s) for s in a.sizes.split(",")):
        seqs = distinct_strings(n)
        s = session.MinHashSession(seqs, K, N_HASH, seed=SEED, reserve=False)
        baseline = n <= a.baseline_max
        say("resident n = %d drawn, %d distinct; queries m = %d%s" % (n, s.n, len(new), "" if baseline else "; the rectangle compare is not run at this size"))
        for bands, rows in BANDINGS:
            rec = {"n": s.n, "m": len(new), "bands": bands, "rows": rows}
            try:
                li, lv = s.lsh_cross_topk(new, bands, rows, TOP)
                r_topk = similarity.mh_lsh_last_route()
                _, lptr, lj, lw = s.lsh_cross_edges(new, bands, rows, THRESHOLD)
                r_edges = similarity.mh_lsh_last_route()
            except da.DynaAlignError as e:
                say("  %3d x %2d: refused: %s" % (bands, rows, e))
                continue
            index = s.lsh_index(bands, rows)
            spare = torch.empty_like(index)
            hold = {}
            legs = [("index build", lambda: device.lsh_index_build(s.sig[:s.n], N_HASH, bands, rows, out=spare)),
                    ("topk query", lambda: s.lsh_cross_topk(new, bands, rows, TOP)),
                    ("edges query", lambda: s.lsh_cross_edges(new, bands, rows, THRESHOLD)),
                    ("topk host", lambda: hold.__setitem__("t", da.similarityMH_lsh_cross_topk(new, seqs, K, N_HASH, bands, rows, TOP, seed=SEED))),
                    ("edges host", lambda: hold.__setitem__("e", da.similarityMH_lsh_cross_edges(new, seqs, K, N_HASH, bands, rows, THRESHOLD, seed=SEED)))]
            if baseline:
                legs += [("rectangle topk", lambda: hold.__setitem__("rt", s.cross_topk(new, TOP))),
                         ("rectangle edges", lambda: hold.__setitem__("re", s.cross_edges(new, threshold=THRESHOLD)))]
            t = alternated(torch, legs, a.reps)
            assert s.lsh_index(bands, rows) is index, "the session built its index again"
            for kept, rebuilt in zip(device.lsh_index_arrays(index, s.n, bands), device.lsh_index_arrays(spare, s.n, bands)):
                assert torch.equal(kept, rebuilt), "a rebuild of the index differs from the kept one"
            assert np.array_equal(hold["t"][0], li) and np.array_equal(hold["e"][2], lj.cpu().numpy()), "host and session routes disagree"
            say("  %3d bands x %2d rows: %d runs in the index (%.1f MB), %d incidences, %d distinct pairs verified, %d list entries (%.2f per row), %d edges"
                % (bands, rows, r_topk["buckets"], index.numel() / 1e6, r_topk["incidences"], r_topk["verified_pairs"], r_topk["edges"],
                   r_topk["edges"] / len(new), r_edges["edges"]))
            for name, _ in legs:
                say("      %-16s %s" % (name, fmt(t[name])))
            rec.update(route_topk=r_topk, route_edges=r_edges, ms=t, index_bytes=int(index.numel()))
            if baseline:
                ri, rv = hold["rt"]
                live = rv > 0
                hit = (ri[:, :, None] == li[:, None, :]).any(2) & live
                _, rptr, rj, _ = hold["re"]
                rows_of = lambda ptr: np.repeat(np.arange(len(new), dtype=np.int64), np.diff(ptr.cpu().numpy()))
                want = rows_of(rptr) * s.n + rj.cpu().numpy()
                got = rows_of(lptr) * s.n + lj.cpu().numpy()
                found = int(np.isin(want, got).sum())
                assert np.isin(got, want).all(), "an LSH edge that the rectangle compare does not have"
                say("      recall@%d against cross_topk (its %d entries with value > 0): %d = %.4f; edges against cross_edges(threshold=%.2f): %d of %d = %.4f"
                    % (TOP, int(live.sum()), int(hit.sum()), hit.sum() / max(int(live.sum()), 1), THRESHOLD, found, len(want), found / max(len(want), 1)))
                rec.update(recall_at_top=float(hit.sum() / max(int(live.sum()), 1)), edge_recall=found / max(len(want), 1))
                for form in ("topk", "edges"):
                    verdicts.append((s.n, bands, rows, form, t[form + " query"]["median"], t["rectangle " + form]["median"]))
            result.append(rec)
            del hold, spare, index
        del s
        torch.cuda.empty_cache()
        _capi.load().da_release_device_memory()
    if verdicts:
        held = all(v[4] < v[5] for v in verdicts)
        say("expectation %s: query against the kept index / rectangle compare, medians in ms: %s"
            % ("CONFIRMED" if held else "REFUTED", "; ".join("%d %dx%d %s %.3f / %.3f" % v for v in verdicts)))
    else:
        say("expectation: not measured (no rectangle compare was run)")
    say("not measured: the rectangle compare at resident sets above --baseline-max; query batches of other sizes; kernel stages; counters; more than one device")
    say(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
