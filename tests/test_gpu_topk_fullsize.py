"""Full-size two-set top-k on ONE MI355X: the 100 000 h3n2-like 20-mers split into two halves (50 000 x 50 000), and the whole set against
itself (100 000 x 100 000: more than 131 068 rows in the joint operand, the raw 32-plane compare), top = 10, n_hash = 500.  A seeded sample
of whole rows is compared with the oracle's counts on the oracle's own signatures; EVERY row is compared with the dense route
(device.similarity_mh_cross in chunks of rows, then torch's stable descending sort) -- indices as integers, values bit for bit."""
import numpy as np
import pytest
import torch

import oracle_lib as O

pytestmark = pytest.mark.gpu

N_ALL, N_HASH, K, SEED, TOP = 100000, 500, 4, 12345, 10


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    from dynaalign_amd import _capi
    assert _capi.load().da_device_count() > 0
    return dynaalign_amd


@pytest.fixture(scope="module")
def seqs():
    from dynaalign_amd import synth
    return synth.to_strings(*synth.h3n2_like(N_ALL, 20))


def check_sample_against_the_oracle(x, y, idx, val, seeds, n_rows, rng):
    rows = np.sort(rng.choice(len(x), n_rows, replace=False))
    sig = O.signatures([x[i] for i in rows] + y, K, N_HASH, seeds)
    cnt = O.mh_counts(sig, 0, n_rows)[:, n_rows:]
    R = cnt.astype(np.float64) / np.float64(N_HASH)                                   # the reference's divide
    want = np.argsort(-R, axis=1, kind="stable")[:, :TOP]
    assert np.array_equal(idx[rows], want), "sampled rows differ from the oracle"
    assert np.array_equal(val[rows].view(np.uint64), np.take_along_axis(R, want, axis=1).view(np.uint64))
    assert int((np.take_along_axis(cnt, want, axis=1)[:, 1:] == np.take_along_axis(cnt, want, axis=1)[:, :-1]).sum()) > 0   # ties were met


def check_every_row_against_the_dense_route(dx_of, dy, m, idx, val, seeds, chunk):
    from dynaalign_amd import device
    for r0 in range(0, m, chunk):
        r1 = min(m, r0 + chunk)
        dense = device.similarity_mh_cross(dx_of(r0, r1), dy, K, N_HASH, seeds)
        v, i = torch.sort(dense, dim=1, descending=True, stable=True)
        v, i = v[:, :TOP].contiguous(), i[:, :TOP].to(torch.int32)
        assert torch.equal(i, idx[r0:r1]), ("indices differ from the dense route in rows", r0, r1)
        assert torch.equal(v.view(torch.int64), val[r0:r1].contiguous().view(torch.int64)), ("values differ in rows", r0, r1)
        del dense, v, i


@pytest.mark.parametrize("shape", ["50000x50000", "100000x100000"])
def test_fullsize_topk(da, seqs, shape):
    from dynaalign_amd import device, _capi
    x, y = (seqs[:N_ALL // 2], seqs[N_ALL // 2:]) if shape == "50000x50000" else (seqs, seqs)
    m = len(x)
    seeds = da.hash_family_seeds(SEED, N_HASH)
    torch.cuda.empty_cache()
    _capi.load().da_release_device_memory()
    dx, dy = device.DeviceSequences(*O.pack(x)), device.DeviceSequences(*O.pack(y))
    idx, val = device.similarity_mh_cross_topk(dx, dy, K, N_HASH, seeds, TOP)
    torch.cuda.synchronize()
    assert idx.shape == (m, TOP) and val.shape == (m, TOP)
    check_sample_against_the_oracle(x, y, idx.cpu().numpy(), val.cpu().numpy(), seeds, 256, np.random.RandomState(len(x)))
    chunk = 5000

    def dx_of(r0, r1):
        return device.DeviceSequences(*O.pack(x[r0:r1]))
    check_every_row_against_the_dense_route(dx_of, dy, m, idx, val, seeds, chunk)
    if shape == "50000x50000":                     # the host boundary and the mirror give the same bits
        hi, hv = da.similarityMH_cross_topk(x, y, K, N_HASH, TOP, seed=SEED)
        assert np.array_equal(hi, idx.cpu().numpy()) and np.array_equal(hv.view(np.uint64), val.cpu().numpy().view(np.uint64))
