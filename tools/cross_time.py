#!/usr/bin/env python3
"""Timing of the two-set MinHash calls on one MI355X (profiles/r06_a_cross_timing.txt).

    python tools/cross_time.py [--reps 20] [--parent-lib PATH] [--out FILE]

Device events, warmed, --reps repetitions per leg, the legs of a comparison alternated in one process; every leg is reported as
min / median / max (the spread).  h3n2-like 20-mers, k = 4, n_hash = 500, seed 12345.

  1  the rectangular float64 kernel against the symmetric one: m = n = 50 000 as rows [0, m) x columns [m_pad, m_pad + n) of the operand
     [x ; filler ; y] (k_mh_compare_r12<true> + its border tiles) against the same 100 000 strings as one square (k_mh_compare_a12<true> +
     its diagonal tiles), duplicate collapse off, 12 planes.  The rectangle has half the tiles and stores each once.
  2  da_dev_similarity_mh_cross (direct route) at m = 16 384, n = 100 000 against the detour the parent commit offers: signatures and planes
     of the concatenation, then da_dev_mh_compare(0, m, symmetric = 0, DA_OUT_F64) into an m x (m + n) buffer.  With --parent-lib the detour
     runs in a child process on THAT library (DYNAALIGN_LIB), so the yardstick is not the code under test; without, on this library.
  3  the duplicate route at m = 20 000, n = 100 000: output bytes per second of the rectangular row expansion against k_expand_stream's on
     the square 100 000 set (DYNAALIGN_MH_EXPAND=rows), and the whole call against the direct route at the same shape.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, N_HASH, SEED = 4, 500, 12345
CROSS = ("da_similarity_mh_cross", "da_similarity_nw_cross", "da_dev_mh_compare_rect", "da_dev_nw_rect", "da_dev_similarity_mh_cross",
         "da_mh_cross_last_route")


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"min": float(a[0]), "median": float(np.median(a)), "max": float(a[-1]), "reps": len(a)}


def fmt(s):
    return "min %8.3f  median %8.3f  max %8.3f ms  (%d reps, spread %.3f ms)" % (s["min"], s["median"], s["max"], s["reps"], s["max"] - s["min"])


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(torch, legs, reps, warm=2):
    """legs: {name: callable}; returns {name: [ms]} with the legs taken in turn"""
    out = {k: [] for k in legs}
    for r in range(warm + reps):
        for name, fn in legs.items():
            ms = timed(torch, fn)
            if r >= warm:
                out[name].append(ms)
    return out


class env:
    def __init__(self, **kw):
        self.kw = {k: str(v) for k, v in kw.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k, v in self.old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def strings(n):
    from dynaalign_amd import synth
    return synth.h3n2_like(n, 20)


def subset(res, off, a, b):
    return res[off[a]:off[b]].copy(), (off[a:b + 1] - off[a]).copy()


def leg_detour(reps, m, n):
    """the parent commit's only route to an m x n cross block (runs on whatever library DYNAALIGN_LIB names)"""
    import torch
    from dynaalign_amd import _capi
    if os.environ.get("DYNAALIGN_LIB"):
        for name in CROSS:                      # the parent library does not have them
            _capi.SIGNATURES.pop(name, None)
    from dynaalign_amd import device
    import dynaalign_amd as da
    res, off = strings(m + n)
    ds = device.DeviceSequences(res, off)
    seeds = torch.from_numpy(da.hash_family_seeds(SEED, N_HASH).view(np.int32).copy()).cuda()
    out = torch.empty((m, m + n), dtype=torch.float64, device="cuda")

    def run():
        _, planes = device.minhash_signatures(ds, K, N_HASH, seeds)
        device.mh_compare(planes, m + n, N_HASH, 0, m, False, _capi.DA_OUT_F64, out=out)
    return alternate(torch, {"detour": run}, reps)["detour"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child-detour", nargs=2, type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--legs", default="1,2,3")
    a = ap.parse_args()
    if a.child_detour:
        print(json.dumps(leg_detour(a.reps, *a.child_detour)))
        return
    import torch
    from dynaalign_amd import _capi, device
    import dynaalign_amd as da
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    seeds_h = da.hash_family_seeds(SEED, N_HASH)
    seeds = torch.from_numpy(seeds_h.view(np.int32).copy()).cuda()
    say("two-set MinHash timing: h3n2-like 20-mers, k = %d, n_hash = %d, %d repetitions per leg after 2 warm-up rounds, device events" % (K, N_HASH, a.reps))
    say("device: %s" % torch.cuda.get_device_name(0))
    legs = set(a.legs.split(","))
    res, off = strings(120000)

    if "1" in legs:
        m = n = 50000
        ds = device.DeviceSequences(*subset(res, off, 0, m + n))
        sig, planes = device.minhash_signatures(ds, K, N_HASH, seeds, min_plane_bits=12)
        m_pad = -(-m // 128) * 128
        joint = torch.empty((m_pad + n, sig.shape[1]), dtype=torch.int32, device="cuda")
        joint[:m] = sig[:m]
        joint[m:m_pad] = sig[:m_pad - m]
        joint[m_pad:] = sig[m:]
        pplanes = device.mh_planes(joint, m_pad + n, N_HASH, min_plane_bits=12)
        sq = torch.empty((m + n, m + n), dtype=torch.float64, device="cuda")
        rc = torch.empty((m, n), dtype=torch.float64, device="cuda")
        t = alternate(torch, {
            "square": lambda: device.mh_compare(planes, m + n, N_HASH, 0, m + n, True, _capi.DA_OUT_F64, out=sq),
            "rect": lambda: device.mh_compare_rect(pplanes, m_pad + n, N_HASH, 0, m, m_pad, m_pad + n, _capi.DA_OUT_F64, out=rc)}, a.reps)
        assert torch.equal(rc.view(torch.int64), sq[:m, m:].contiguous().view(torch.int64))
        s_sq, s_rc = stats(t["square"]), stats(t["rect"])
        say()
        say("1  rectangle against square (planes: %d / %d bits)" % (planes.bits, pplanes.bits))
        say("   square 100 000 x 100 000, k_mh_compare_a12<true>     : " + fmt(s_sq))
        say("   rect    50 000 x  50 000, k_mh_compare_r12<true>     : " + fmt(s_rc))
        say("   rect / square (medians) = %.4f; bar: rect <= square / 2 + spread of the square leg = %.3f ms -> %s"
            % (s_rc["median"] / s_sq["median"], s_sq["median"] / 2 + (s_sq["max"] - s_sq["min"]),
               "met" if s_rc["median"] <= s_sq["median"] / 2 + (s_sq["max"] - s_sq["min"]) else "NOT met"))
        say("   output: square %.2f TB/s, rect %.2f TB/s" % ((m + n) ** 2 * 8 / s_sq["median"] / 1e9, m * n * 8 / s_rc["median"] / 1e9))
        del sq, rc, planes, pplanes, joint, sig, ds
        torch.cuda.empty_cache()
        _capi.load().da_release_device_memory()

    if "2" in legs:
        m, n = 16384, 100000
        dx = device.DeviceSequences(*subset(res, off, 0, m))
        dy = device.DeviceSequences(*subset(res, off, m, m + n))
        out = torch.empty((m, n), dtype=torch.float64, device="cuda")
        with env(DYNAALIGN_MH_NO_DEDUP=1):
            t_new = alternate(torch, {"cross": lambda: device.similarity_mh_cross(dx, dy, K, N_HASH, seeds, out=out)}, a.reps)["cross"]
            route = device.mh_cross_last_route()
        del out
        torch.cuda.empty_cache()
        _capi.load().da_release_device_memory()
        child_env = dict(os.environ)
        if a.parent_lib:
            child_env["DYNAALIGN_LIB"] = os.path.abspath(a.parent_lib)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--child-detour", str(m), str(n)],
                           env=child_env, stdout=subprocess.PIPE, timeout=600)
        if p.returncode != 0:
            raise SystemExit("the detour's child process failed (%d)" % p.returncode)
        t_old = json.loads(p.stdout.decode().strip().splitlines()[-1])
        s_new, s_old = stats(t_new), stats(t_old)
        say()
        say("2  the one call against the detour, m = %d, n = %d (direct route, %d planes; phases of the last call: plan %.2f, K1 + K1b %.2f, K2 %.2f ms)"
            % (m, n, route["plane_bits"], route["plan_ms"], route["codes_ms"], route["k2_ms"]))
        say("   da_dev_similarity_mh_cross                          : " + fmt(s_new))
        say("   detour (%s): K1 + K1b on c(x, y), da_dev_mh_compare(0, m, symmetric = 0, F64) into m x (m + n)"
            % ("library of the parent commit, child process" if a.parent_lib else "this library, child process"))
        say("                                                       : " + fmt(s_old))
        say("   detour / cross (medians) = %.3f; cross max %.3f %s detour min %.3f"
            % (s_old["median"] / s_new["median"], s_new["max"], "<" if s_new["max"] < s_old["min"] else ">=", s_old["min"]))

    if "3" in legs:
        m, n = 20000, 100000
        dx = device.DeviceSequences(*subset(res, off, 0, m))
        dy = device.DeviceSequences(*subset(res, off, m, m + n))
        dsq = device.DeviceSequences(*subset(res, off, 0, n))
        out = torch.empty((m, n), dtype=torch.float64, device="cuda")
        sq = torch.empty((n, n), dtype=torch.float64, device="cuda")
        rect_ms, sq_ms, routes = [], [], {}

        def dup():
            device.similarity_mh_cross(dx, dy, K, N_HASH, seeds, out=out)
            routes["dup"] = device.mh_cross_last_route()
            rect_ms.append(routes["dup"]["expand_ms"])

        def direct():
            with env(DYNAALIGN_MH_NO_DEDUP=1):
                device.similarity_mh_cross(dx, dy, K, N_HASH, seeds, out=out)

        def square():
            with env(DYNAALIGN_MH_EXPAND="rows"):
                device.similarity_mh(dsq, K, N_HASH, seeds, out=sq)
                r = device.mh_last_route()
            assert r["expansion"] == "rows", r
            sq_ms.append(r["expand_ms"])
        t = alternate(torch, {"dup": dup, "direct": direct, "square": square}, a.reps)
        rect_ms, sq_ms = rect_ms[2:], sq_ms[2:]
        r = routes["dup"]
        assert r["dedup"], r
        s_r, s_s = stats(rect_ms), stats(sq_ms)
        say()
        say("3  duplicate route, m = %d, n = %d: %d x %d unique strings" % (m, n, r["unique_x"], r["unique_y"]))
        say("   rectangular expansion (k_expand_stream, %d x %d)    : " % (m, n) + fmt(s_r) + "  -> %.2f TB/s" % (m * n * 8 / s_r["median"] / 1e9))
        say("   square expansion (k_expand_stream, %d x %d) : " % (n, n) + fmt(s_s) + "  -> %.2f TB/s" % (n * n * 8 / s_s["median"] / 1e9))
        say("   whole call, duplicate route                         : " + fmt(stats(t["dup"])))
        say("   whole call, direct route                            : " + fmt(stats(t["direct"])))
        say("   phases of the last duplicate call: plans %.2f, K1 + K1b %.2f, K2 %.2f, copy lists %.2f, expansion %.2f ms"
            % (r["plan_ms"], r["codes_ms"], r["k2_ms"], r["lists_ms"], r["expand_ms"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
