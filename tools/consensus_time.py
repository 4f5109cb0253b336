#!/usr/bin/env python3
"""Timing of the device consensus against the host loop of clusterconsensus on one MI355X (profiles/r24_a_consensus_timing.txt; DESIGN.md
section 7).

    python tools/consensus_time.py [--reps 5] [--n 100000] [--baseline-pairs 8000000] [--no-baseline] [--one-call] [--out FILE]

Input: clusterbreak(size_max=800, session=s, louvain="device") on h3n2-like 20-mers (k = 4, n_hash = 500, seed 12345, thresh_p = .8); the
consensus of its result.  Host clock around calls that end in a device synchronise, 1 warm-up call, --reps timed calls per leg, the legs
alternated in one process; every leg is reported as min / median / max.

  a  the device route at its three boundaries: device.cluster_consensus on the resident pooled table (da_dev_cluster_consensus), the C
     boundary da_cluster_consensus on packed host arrays, and clusterconsensus_device(result)
  b  the baseline, clusterconsensus(rows) as the parent commit has it, against clusterconsensus_device on the SAME rows.  The whole result
     would keep the host loop busy for minutes, so the rows are those of the first clusters (first-appearance order) whose ordered
     in-cluster pairs stay within --baseline-pairs; the baseline runs once, without a warm-up, and the output says so

--one-call runs a single device.cluster_consensus on the whole result and nothing else: the run to put under a kernel trace for the time
per kernel.  Expectation to confirm or refute: the device route is faster than the host loop by more than an order of magnitude, and the
alignment kernels, not the consensus kernels, take most of its device time.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, N_HASH, SEED = 4, 500, 12345


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"min": float(a[0]), "median": float(np.median(a)), "max": float(a[-1]), "reps": len(a)}


def fmt(s):
    return "min %10.3f  median %10.3f  max %10.3f ms  (%d reps)" % (s["min"], s["median"], s["max"], s["reps"])


def alternate(torch, legs, reps, warm=1):
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


def pool_of(rows):
    """rows -> (members cluster after cluster, cluster_ptr, cluster_of per pooled member): clusters of two or more, first-appearance order"""
    members = {}
    for seq, cid in rows:
        members.setdefault(cid, []).append(seq)
    seqs, ptr, cl = [], [0], []
    for k, mem in enumerate(m for m in members.values() if len(m) > 1):
        seqs += mem
        cl += [k] * len(mem)
        ptr.append(len(seqs))
    return seqs, np.array(ptr, np.int64), np.array(cl, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--baseline-pairs", type=int, default=8000000)
    ap.add_argument("--no-baseline", action="store_true", help="skip leg b")
    ap.add_argument("--one-call", action="store_true", help="one device.cluster_consensus on the whole result, nothing else")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import dynaalign_amd as da
    from dynaalign_amd import device, session, synth, _capi
    lib = _capi.load()
    if lib.da_device_count() <= 0:
        raise SystemExit("no GPU: nothing is measured")
    seqs = synth.to_strings(*synth.h3n2_like(a.n, 20))
    s = session.MinHashSession(seqs, K, N_HASH, seed=SEED)
    res = da.clusterbreak(seqs, size_max=800, thresh_p=0.8, session=s, louvain="device")
    del s
    torch.cuda.empty_cache()
    rows = [(str(r[0]), r[1]) for r in res["clustered_seq"]]
    pool, ptr, cl = pool_of(rows)
    sizes = np.diff(ptr)
    pairs, vote_rows = int((sizes * (sizes - 1)).sum()), int((sizes - 1).sum())
    ds = device.DeviceSequences(*da.pack_sequences(pool))
    device.nw_encode(ds)
    if a.one_call:
        device.cluster_consensus(ds, ptr)
        torch.cuda.synchronize()
        return
    lines, result = [], {}

    def say(t=""):
        print(t, flush=True)
        lines.append(t)

    say("device consensus, h3n2-like 20-mers, N = %d: %d clustered rows, %d clusters of two or more (largest %d) with %d members, %d ordered pairs, "
        "%d vote rows; 1 warm-up + %d timed calls per leg, legs alternated" % (a.n, len(rows), len(sizes), int(sizes.max()), len(pool), pairs, vote_rows, a.reps))
    work = torch.empty(device.cluster_consensus_workspace_bytes(ptr, ds.max_len), dtype=torch.uint8, device="cuda")
    say("   workspace %.2f GB (blocks of up to 2^20 pairs)" % (work.numel() / 1e9))
    pres, poff = da.pack_sequences(pool)
    ld = max(int(np.diff(poff).max()), 1)
    cons, cons_len, cen = np.zeros((len(sizes), ld), np.uint8), np.zeros(len(sizes), np.int32), np.zeros(len(sizes), np.int32)

    def c_boundary():
        _capi.check(lib.da_cluster_consensus(pres.ctypes.data, poff.ctypes.data, len(pool), cl.ctypes.data, len(sizes), b"BLOSUM62", 10, 4,
                                             cons.ctypes.data, ld, cons_len.ctypes.data, cen.ctypes.data))

    keep = {}
    r = alternate(torch, {"device.cluster_consensus (resident pool)": lambda: keep.update(dev=device.cluster_consensus(ds, ptr, work=work)),
                          "da_cluster_consensus (packed host arrays)": c_boundary,
                          "clusterconsensus_device(result)": lambda: keep.update(py=da.clusterconsensus_device(res))}, a.reps)
    say("a  the device route")
    for k_, v in r.items():
        say("     %-44s %s" % (k_, fmt(v)))
    dev_ms = r["device.cluster_consensus (resident pool)"]["median"]
    say("     pairs aligned per second at the device boundary: %.3g (both phases: %d alignments)" % ((pairs + vote_rows) / dev_ms * 1e3, pairs + vote_rows))
    dcons, dlen, _ = keep["dev"]
    dcons, dlen = dcons.cpu().numpy(), dlen.cpu().numpy()
    count = {}
    for _, cid in rows:
        count[cid] = count.get(cid, 0) + 1
    py = [c.encode("latin-1") for cid, c in keep["py"] if count[cid] > 1]
    same = all(bytes(dcons[k][:dlen[k]]) == bytes(cons[k][:cons_len[k]]) == py[k] for k in range(len(sizes)))
    say("     the three boundaries agree: %s" % same)
    result["a"] = {"timing": r, "pairs": pairs, "vote_rows": vote_rows, "clusters": len(sizes), "members": len(pool), "largest": int(sizes.max())}
    del work
    torch.cuda.empty_cache()
    if not a.no_baseline:
        ids, used = {}, 0
        for _, cid in rows:                               # first-appearance order
            if cid in ids:
                continue
            c = count[cid]
            if used + c * (c - 1) > a.baseline_pairs:
                break
            ids[cid] = True
            used += c * (c - 1)
        sub = [row for row in rows if row[1] in ids]
        t = time.perf_counter()
        base = da.clusterconsensus(sub)
        base_ms = (time.perf_counter() - t) * 1e3
        got = {}
        rd = alternate(torch, {"clusterconsensus_device (same rows)": lambda: got.update(v=da.clusterconsensus_device(sub))}, a.reps)
        say("b  the baseline on the first %d clusters (%d rows, %d ordered pairs = %.1f %% of all): the whole result would take the host loop minutes"
            % (len(ids), len(sub), used, 100.0 * used / max(pairs, 1)))
        say("     %-44s %10.3f ms  (1 run, no warm-up)" % ("clusterconsensus (host loop, parent commit)", base_ms))
        say("     %-44s %s" % ("clusterconsensus_device (same rows)", fmt(rd["clusterconsensus_device (same rows)"])))
        say("     equal results: %s;  host loop / device route %.1f;  the host loop extrapolated to all pairs: %.0f s"
            % (base == got["v"], base_ms / rd["clusterconsensus_device (same rows)"]["median"], base_ms / 1e3 * pairs / max(used, 1)))
        result["b"] = {"clusters": len(ids), "rows": len(sub), "pairs": used, "baseline_ms": base_ms, "device": rd, "equal": base == got["v"]}
    say(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
