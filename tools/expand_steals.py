#!/usr/bin/env python3
"""Where the pipelined row expansion's workgroups find their items: per chunk launch and XCD, the items taken from the XCD's own zone and from
other zones, for both id orders of the duplicate plan, on the headline input (100k h3n2-like).  Needs the counting build of the library:
   tools/experiments/build_steal_count.sh && DYNAALIGN_LIB=tools/experiments/lib/libsteals.so python3 tools/expand_steals.py"""
import ctypes, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np, torch
import dynaalign_amd as da
from dynaalign_amd import _capi, device, synth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
res, off = synth.h3n2_like(n, 20)
ds = device.DeviceSequences(res, off)
seeds = da.hash_family_seeds(12345, 500)
out = torch.empty((n, n), dtype=torch.float64, device="cuda")


def steals(reset):
    fn = _capi.load().da_debug_expand_steals
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_int], ctypes.c_int
    a = np.zeros((64, 8, 2), np.uint32)
    assert fn(a.ctypes.data, reset) == 0
    return a.astype(np.int64)


for order in ("first", "zoned"):
    os.environ["DYNAALIGN_MH_DEDUP_ORDER"] = order
    for _ in range(3):
        device.similarity_mh(ds, 4, 500, seeds, out=out)
    torch.cuda.synchronize()
    steals(1)
    calls = 5
    for _ in range(calls):
        device.similarity_mh(ds, 4, 500, seeds, out=out)
    torch.cuda.synchronize()
    a = steals(1)
    r = device.mh_last_route()
    print("order %s: %s, %d launches, items per call %.0f (own zone %.0f, other zones %.0f)"
          % (order, r["expansion"], r["chunks"], a.sum() / calls, a[:, :, 0].sum() / calls, a[:, :, 1].sum() / calls))
    print("  launch (bands done) | per XCD 0 .. 7: own zone / other zones (mean of %d calls)" % calls)
    for b in np.flatnonzero(a.sum(axis=(1, 2))):
        print("  %2d | %s" % (b, "  ".join("%4.0f/%-4.0f" % (a[b, x, 0] / calls, a[b, x, 1] / calls) for x in range(8))))
    del os.environ["DYNAALIGN_MH_DEDUP_ORDER"]
