"""Full-size two-set MinHash on ONE MI355X: m = 20 000 against n = 100 000 (rows 0 .. 19 999 of the 120 000 h3n2-like 20-mers against
the rest), the whole 16 GB result of the direct route, the duplicate route and da_dev_mh_compare_rect on an operand built here compared
on the device, 200+ whole rows against the oracle's compare loop on the oracle's own signatures, and the transposed call
(m = 100 000, n = 20 000) against the transpose."""
import os

import numpy as np
import pytest
import torch

import oracle_lib as O

pytestmark = pytest.mark.gpu

M, N, N_HASH, K, SEED = 20000, 100000, 500, 4, 12345


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    from dynaalign_amd import _capi
    assert _capi.load().da_device_count() > 0
    return dynaalign_amd


def _same_bits(a, b, step=4000):
    for r0 in range(0, a.shape[0], step):
        x, y = a[r0:r0 + step].view(torch.int64), b[r0:r0 + step].view(torch.int64)
        if not torch.equal(x, y):
            bad = (x != y).nonzero()[0].tolist()
            raise AssertionError("first difference at (%d, %d): %r vs %r" % (r0 + bad[0], bad[1], a[r0 + bad[0], bad[1]].item(),
                                                                             b[r0 + bad[0], bad[1]].item()))


def test_20000_against_100000_every_route(da):
    from dynaalign_amd import device, synth, _capi
    res, off = synth.h3n2_like(M + N, 20)
    seqs = synth.to_strings(res, off)
    x, y = seqs[:M], seqs[M:]
    seeds = da.hash_family_seeds(SEED, N_HASH)
    dx, dy = device.DeviceSequences(*O.pack(x)), device.DeviceSequences(*O.pack(y))
    torch.cuda.empty_cache()
    _capi.load().da_release_device_memory()
    ref = torch.empty((M, N), dtype=torch.float64, device="cuda")
    out = torch.empty((M, N), dtype=torch.float64, device="cuda")

    def call(a, b, o, **env):
        os.environ.update({k: str(v) for k, v in env.items()})
        try:
            o.fill_(-1.0)
            device.similarity_mh_cross(a, b, K, N_HASH, seeds, out=o)
            torch.cuda.synchronize()
            return device.mh_cross_last_route()
        finally:
            for k in env:
                del os.environ[k]
    route = call(dx, dy, ref, DYNAALIGN_MH_NO_DEDUP=1)
    assert not route["dedup"] and route["plane_bits"] in (12, 14, 15, 16), route     # dictionary codes: 120 064 rows fit them
    # 200+ whole rows (first, middle and last tiles of x; tile edges included) against the oracle's counts on the oracle's signatures
    sig = O.signatures(seqs, K, N_HASH, seeds)
    ratio = np.arange(N_HASH + 1, dtype=np.float64) / N_HASH                 # the reference's divide, on the host
    checked = 0
    for a in (0, 96, 9984 - 17, M // 2 + 120, M - 128 - 20, M - 40):
        b = min(M, a + 40)
        want = O.mh_counts(sig, a, b)[:, M:]
        blk = ref[a:b].cpu().numpy()
        cnt = np.searchsorted(ratio, blk)
        assert np.array_equal(ratio[np.minimum(cnt, N_HASH)], blk)            # every element IS one of the ratios
        assert np.array_equal(cnt.astype(np.uint16), want), "match counts differ from the oracle in rows %d..%d" % (a, b)
        checked += b - a
    assert checked >= 200
    # the duplicate route, by the built-in rule, over the whole result
    route = call(dx, dy, out)
    assert route["dedup"] and (route["unique_x"], route["unique_y"]) == (len(set(x)), len(set(y))), route
    _same_bits(out, ref)
    # da_dev_mh_compare_rect on the caller's operand: c(x, y) as it is (rows [0, M) x columns [M, M + N): M is not a multiple of 128, the
    # compiled kernel) and with x padded to a multiple of 128 rows (the hand-scheduled kernel)
    dxy = device.DeviceSequences(res, off)
    sig_d, planes = device.minhash_signatures(dxy, K, N_HASH, seeds)
    out.fill_(-1.0)
    device.mh_compare_rect(planes, M + N, N_HASH, 0, M, M, M + N, _capi.DA_OUT_F64, out=out)
    _same_bits(out, ref)
    del planes
    m_pad = -(-M // 128) * 128
    joint = torch.empty((m_pad + N, sig_d.shape[1]), dtype=torch.int32, device="cuda")
    joint[:M] = sig_d[:M]
    joint[M:m_pad] = sig_d[:m_pad - M]
    joint[m_pad:] = sig_d[M:]
    pplanes = device.mh_planes(joint, m_pad + N, N_HASH)
    out.fill_(-1.0)
    device.mh_compare_rect(pplanes, m_pad + N, N_HASH, 0, M, m_pad, m_pad + N, _capi.DA_OUT_F64, out=out)
    _same_bits(out, ref)
    cnt16 = device.mh_compare_rect(pplanes, m_pad + N, N_HASH, 0, M, m_pad, m_pad + N, _capi.DA_OUT_COMPACT)
    device.widen(cnt16, False, N_HASH, out=out)
    _same_bits(out, ref)
    del cnt16, pplanes, joint, sig_d, out
    torch.cuda.empty_cache()
    # the transposed call: y against x, both routes, against the transpose
    out_t = torch.empty((N, M), dtype=torch.float64, device="cuda")
    ref_t = ref.t()
    for env, dedup in (({"DYNAALIGN_MH_NO_DEDUP": 1}, False), ({}, True)):
        route = call(dy, dx, out_t, **env)
        assert route["dedup"] == dedup and (route["m"], route["n"]) == (N, M), route
        for r0 in range(0, N, 10000):
            assert torch.equal(out_t[r0:r0 + 10000].view(torch.int64), ref_t[r0:r0 + 10000].contiguous().view(torch.int64)), (env, r0)
