"""GPU tests of the two-set MinHash LSH form (the index and the probe of lsh_cross_kernels.hip, the back end of lsh_kernels.hip): similarityMH_lsh_cross_edges / _topk, the device pieces
(da_dev_lsh_index_build / _probe, da_dev_lsh_cross_verify_pairs / _edges / _topk) and MinHashSession.lsh_index / lsh_cross_edges /
lsh_cross_topk.  Every comparison is exact -- indices as integers, weights as uint64 bit patterns -- against test_lsh_cross_cpu.cross_model
(the i < m <= j block of the one-set model on the stacked signatures) or, where a bucket is too large for a Python model, against the numpy
definitions that test_lsh_cross_cpu.py checks against that model."""
import numpy as np
import pytest
import torch

from test_gpu_jaccard import family
from test_gpu_lsh import CASES, SEED, oracle_sig, random_sig, to_device
from test_lsh_cpu import FIXED, planted
from test_lsh_cross_cpu import cross_model, same_cross_edges, same_cross_lists, topk_model

pytestmark = pytest.mark.gpu

UNSUPPORTED, BAD_ARG = 10, 11


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    from dynaalign_amd import _capi
    assert _capi.load().da_device_count() > 0
    return dynaalign_amd


def weights(count, n_hash):
    return count.cpu().numpy().view(np.uint16).astype(np.float64) / np.float64(n_hash)


def device_cross(sig_x, sig_y, bands, rows, thr, ld_x=None, ld_y=None, top=None, **kw):
    """the device entries on host signatures: (i, j, w) of lsh_cross_edges, or (idx, val) of lsh_cross_topk when top is given"""
    from dynaalign_amd import device
    n_hash = sig_x.shape[1]
    tx, ty = to_device(sig_x, ld_x), to_device(sig_y, ld_y)
    index = device.lsh_index_build(ty, n_hash, bands, rows)
    if top is None:
        i, j, c = device.lsh_cross_edges(index, tx, ty, n_hash, bands, rows, thr, **kw)
        torch.cuda.synchronize()
        return i.cpu().numpy(), j.cpu().numpy(), weights(c, n_hash)
    idx, key = device.lsh_cross_topk(index, tx, ty, n_hash, bands, rows, top, threshold=thr, **kw)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), weights(key, n_hash)


def check_route(want, written):
    from dynaalign_amd import similarity
    route = similarity.mh_lsh_last_route()
    assert route == {"buckets": want["buckets"], "incidences": want["incidences"], "verified_pairs": len(want["pairs"]), "edges": written}


# ---- the host entries against the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params,fam", CASES, ids=["12x4", "10x5", "33x3", "1x64", "40x1"])
def test_host_entries_equal_the_model_on_oracle_signatures(da, params, fam):
    k, n_hash, bands, rows, thr = params
    seqs = family(*fam)
    half = len(seqs) // 2
    x, y = seqs[:half] + FIXED, seqs[half:] + FIXED        # empty, one-residue and byte-identical strings across the two sets
    sig_x, sig_y = oracle_sig(x, k, n_hash), oracle_sig(y, k, n_hash)
    want = cross_model(sig_x, sig_y, bands, rows, thr)
    # what the inputs were chosen for
    assert want["incidences"] > 0 and len(want["i"]) > 0 and (len(x) - 1, len(y) - 1) in want["pairs"]
    s = (sig_x[:, None, :] == sig_y[None, :, :]).sum(2).astype(np.float64) / np.float64(n_hash)
    must_not_add = set(zip(*(a.tolist() for a in np.nonzero((s >= thr) & (s > 0))))) - want["pairs"]
    if bands > 1:
        assert want["multi"] > 0 and want["below"] > 0
    if rows > 1:
        assert len(must_not_add) > 0
    if rows == 1:
        assert want["largest"] > 16                        # a probed run of more than a few rows
    got_thr, i, j, w = da.similarityMH_lsh_cross_edges(x, y, k, n_hash, bands, rows, thr, seed=SEED)
    assert got_thr == thr
    same_cross_edges((i, j, w), want)
    assert not (set(zip(i.tolist(), j.tolist())) & must_not_add)
    check_route(want, len(i))
    for top in (1, 10):
        want_idx, want_val = topk_model(want, len(x), top)
        same_cross_lists(da.similarityMH_lsh_cross_topk(x, y, k, n_hash, bands, rows, top, threshold=thr, seed=SEED), want_idx, want_val)
        check_route(want, sum(1 for r in want_idx for t in r if t >= 0))
    # the numpy definition on the library's own signatures agrees as well
    lib_x, lib_y = da.minhash_signatures(x, k, n_hash, seed=SEED), da.minhash_signatures(y, k, n_hash, seed=SEED)
    same_cross_edges(da.lsh_cross_edges_dense(lib_x, lib_y, bands, rows, thr), want)


def test_one_query_and_one_resident_sequence(da):
    a, near, far = "ACDEFGHIKLMNPQRSTVWY", "ACDEFGHIKLMNPQRSTVWW", "WWWWWYYYYYWWWWWYYYYY"
    for x, y in (([a], [near]), ([a], [far]), ([a], [a]), ([a], [far, near, a]), ([far, near, a], [a]), ([""], [""])):
        want = cross_model(oracle_sig(x, 4, 48), oracle_sig(y, 4, 48), 12, 4, 0.5)
        _, i, j, w = da.similarityMH_lsh_cross_edges(x, y, 4, 48, 12, 4, 0.5, seed=SEED)
        same_cross_edges((i, j, w), want)
        same_cross_lists(da.similarityMH_lsh_cross_topk(x, y, 4, 48, 12, 4, 3, threshold=0.5, seed=SEED), *topk_model(want, len(x), 3))
    assert len(i) == 1 and w[0] == 1.0                       # two empty strings: equal signatures
    _, i, _, _ = da.similarityMH_lsh_cross_edges([a], [far, near, a], 4, 48, 12, 4, 0.5, seed=SEED)
    assert i.tolist() == [0, 0]                              # the near duplicate and the copy


# ---- the device entries on synthetic signatures -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_hash,bands,rows", [(1, 1, 1), (31, 5, 6), (31, 31, 1), (33, 1, 33), (33, 4, 8), (48, 12, 4), (48, 2, 17), (200, 3, 65),
                                               (600, 9, 64)])
def test_device_edges_and_lists_on_planted_signatures(da, n_hash, bands, rows):
    """random signatures with planted agreements, values 0 and 0xFFFFFFFF among them, split into x and y; two buffers with different
    leading dimensions, both larger than n_hash, whose padding columns hold one equal value"""
    sig = planted(n_hash, 150, n_hash, bands, rows)
    sig[::7, ::3] = 0
    sig[3::11] = 0xFFFFFFFF
    sig[5::11] = 0
    sig_x, sig_y = sig[:63], sig[63:]
    for thr in (0.0, 0.5, 1.0):
        want = cross_model(sig_x, sig_y, bands, rows, thr)
        assert want["incidences"] > 0
        same_cross_edges(device_cross(sig_x, sig_y, bands, rows, thr, ld_x=n_hash + 5, ld_y=n_hash + 9), want)
        check_route(want, len(want["i"]))
        if thr == 0.5:
            same_cross_lists(device_cross(sig_x, sig_y, bands, rows, thr, ld_x=n_hash + 9, ld_y=n_hash + 5, top=4), *topk_model(want, len(sig_x), 4))


def test_keys_outside_the_index_and_a_batch_without_any_candidate(da):
    from dynaalign_amd import device, similarity
    n_hash, bands, rows = 12, 3, 4
    sig_y, sig_x = random_sig(21, 3, n_hash), random_sig(22, 200, n_hash)
    ty, tx = to_device(sig_y, 16), to_device(sig_x, 20)
    ky = device.lsh_band_keys(ty, n_hash, bands, rows)[0].cpu().numpy().view(np.uint64)
    kx = device.lsh_band_keys(tx, n_hash, bands, rows)[0].cpu().numpy().view(np.uint64)
    for t in range(bands):                                   # in every band some x key sorts in front of the band's segment and some behind it
        assert (kx[:, t] < ky[:, t].min()).any() and (kx[:, t] > ky[:, t].max()).any()
    index = device.lsh_index_build(ty, n_hash, bands, rows)
    lo, ln = device.lsh_index_probe(index, 3, tx, n_hash, bands, rows)
    _, band_start, keys, _ = device.lsh_index_arrays(index, 3, bands)
    assert band_start.cpu().tolist() == [0, 3, 6, 9] and np.array_equal(keys.cpu().numpy().view(np.uint64), np.sort(ky.ravel()))
    assert int(ln.abs().sum()) == 0
    lo, skeys = lo.cpu().numpy(), np.sort(ky.ravel())
    assert np.array_equal(lo, np.searchsorted(skeys, kx.ravel()).reshape(kx.shape))   # where the key would stand: 3 t .. 3 t + 3
    assert (lo == 0).any() and (lo == 9).any()
    i, j, c = device.lsh_cross_edges(index, tx, ty, n_hash, bands, rows, 0.0, max_candidates=0)
    assert i.numel() == j.numel() == c.numel() == 0
    assert similarity.mh_lsh_last_route() == {"buckets": 9, "incidences": 0, "verified_pairs": 0, "edges": 0}
    idx, key = device.lsh_cross_topk(index, tx, ty, n_hash, bands, rows, 5, max_candidates=0)
    assert idx.shape == key.shape == (200, 5) and bool((idx == -1).all()) and bool((key == 0).all())
    assert similarity.mh_lsh_last_route()["edges"] == 0


@pytest.fixture(scope="module")
def big_buckets(built):
    """y with a bucket of 2 100 rows (band 0 of A), one of 300 (band 1 of B) and one of 40 (band 2 of C) -- counts vary inside them -- and
    x rows that find the one, the other, two of them at once, or nothing; some x rows are identical.  n_hash 16 = 3 bands of 4 + 4 tail
    columns.  The references are the numpy definitions."""
    import dynaalign_amd as da
    rng = np.random.RandomState(77)
    n_hash, bands, rows = 16, 3, 4
    a, b, c = (rng.randint(0, 1 << 32, n_hash, dtype=np.uint64).astype(np.uint32) for _ in range(3))

    def near(base, band, count):
        out = rng.randint(0, 1 << 32, (count, n_hash), dtype=np.uint64).astype(np.uint32)
        copy = rng.rand(count, n_hash) < 0.4                 # other columns of the base too: the counts differ from row to row
        out[copy] = np.tile(base, (count, 1))[copy]
        out[:, band * rows:(band + 1) * rows] = base[band * rows:(band + 1) * rows]
        return out
    sig_y = np.vstack([near(a, 0, 2100), near(b, 1, 300), near(c, 2, 40), rng.randint(0, 1 << 32, (60, n_hash), dtype=np.uint64).astype(np.uint32)])
    sig_y = sig_y[rng.permutation(len(sig_y))]
    ab = a.copy()
    ab[4:8] = b[4:8]                                         # the bucket of A and the bucket of B
    sig_x = np.vstack([a, b, c, ab, near(a, 0, 3), near(b, 1, 2), near(c, 2, 2), a, ab,
                       rng.randint(0, 1 << 32, (5, n_hash), dtype=np.uint64).astype(np.uint32)])
    i, j, w = da.lsh_cross_edges_dense(sig_x, sig_y, bands, rows, 0.0)
    deg = np.bincount(i, minlength=len(sig_x))
    # x rows in all three classes of the selection: up to 64 entries, up to 2 048, more
    assert (deg == 0).sum() >= 5 and ((deg > 0) & (deg <= 64)).sum() >= 3 and ((deg > 64) & (deg <= 2048)).sum() >= 3 and (deg > 2048).sum() >= 2
    assert deg[0] == deg[11] >= 2100 and deg[3] == deg[12] >= 2400
    return sig_x, sig_y, (n_hash, bands, rows), (i, j, w)


def test_buckets_larger_than_a_workgroup_and_identical_queries(da, big_buckets):
    sig_x, sig_y, (n_hash, bands, rows), (wi, wj, ww) = big_buckets
    i, j, w = device_cross(sig_x, sig_y, bands, rows, 0.0, ld_x=20, ld_y=24)
    assert np.array_equal(i, wi) and np.array_equal(j, wj) and np.array_equal(w.view(np.uint64), ww.view(np.uint64))
    # identical x rows get identical partner lists
    assert np.array_equal(j[i == 0], j[i == 11]) and np.array_equal(j[i == 3], j[i == 12]) and (i == 3).sum() >= 2400
    ti, tj, tw = da.lsh_cross_edges_dense(sig_x, sig_y, bands, rows, 0.5)
    i, j, w = device_cross(sig_x, sig_y, bands, rows, 0.5)
    assert 0 < len(ti) < len(wi)
    assert np.array_equal(i, ti) and np.array_equal(j, tj) and np.array_equal(w.view(np.uint64), tw.view(np.uint64))


@pytest.mark.parametrize("top", [1, 10, 1024])
def test_lists_of_rows_in_all_three_selection_classes(da, big_buckets, top):
    sig_x, sig_y, (n_hash, bands, rows), _ = big_buckets
    for thr in (0.0, 0.5):
        want_idx, want_val = da.lsh_cross_topk_dense(sig_x, sig_y, bands, rows, top, thr)
        idx, val = device_cross(sig_x, sig_y, bands, rows, thr, ld_x=24, ld_y=20, top=top)
        assert idx.dtype == np.int32 and idx.shape == (len(sig_x), top)
        assert np.array_equal(idx, want_idx) and np.array_equal(val.view(np.uint64), want_val.view(np.uint64))
    if top == 1024:
        assert (idx[0] >= 0).all() and (idx[7:11] >= 0).sum(1).max() < 1024 and (idx[-1] == -1).all()


def test_tail_columns_count_but_make_no_candidate_and_bands_dedup(da):
    n_hash, bands, rows = 48, 10, 4                        # columns 40 .. 47 belong to no band
    sig_x, sig_y = random_sig(3, 4, n_hash), random_sig(4, 4, n_hash)
    sig_y[0, 40:] = sig_x[0, 40:]                          # agreement in the tail only: no candidate
    sig_y[1, 36:40] = sig_x[1, 36:40]                      # the last band only
    sig_y[2, 0:4] = sig_x[2, 0:4]                          # band 0 and the last band: one edge
    sig_y[2, 36:40] = sig_x[2, 36:40]
    sig_y[3, 0:4] = sig_x[3, 0:4]                          # a candidate whose tail counts towards the threshold
    sig_y[3, 40:] = sig_x[3, 40:]
    want = cross_model(sig_x, sig_y, bands, rows, 0.0)
    assert (0, 0) not in want["pairs"] and want["bands_of"][(1, 1)] == [9] and want["bands_of"][(2, 2)] == [0, 9]
    i, j, w = device_cross(sig_x, sig_y, bands, rows, 0.0, ld_x=64, ld_y=50)
    same_cross_edges((i, j, w), want)
    check_route(want, 3)
    assert want["incidences"] == 4 and want["buckets"] == 40
    assert list(zip(i.tolist(), j.tolist(), w.tolist())) == [(1, 1, 4 / 48), (2, 2, 8 / 48), (3, 3, 12 / 48)]
    # the threshold is applied to the whole count: 12 / 48 passes 0.25, 8 / 48 does not
    i, j, w = device_cross(sig_x, sig_y, bands, rows, 0.25)
    assert list(zip(i.tolist(), j.tolist(), w.tolist())) == [(3, 3, 12 / 48)]
    idx, val = device_cross(sig_x, sig_y, bands, rows, 0.25, top=2)
    assert idx.tolist() == [[-1, -1], [-1, -1], [-1, -1], [3, -1]] and val.tolist() == [[0.0, 0.0]] * 3 + [[12 / 48, 0.0]]


def test_one_set_equals_two_sets_on_itself(da):
    """The back end is one set of kernels with two enumerations of the slots: a set queried against its own index must give the one-set
    result twice over -- every pair in both directions -- plus the diagonal.  70 copies of row 0 make a bucket of 71 rows in every band:
    some chunks of 64 slots hold a single i, and one i's slots cross chunk boundaries."""
    from dynaalign_amd import device, similarity
    n_hash, bands, rows = 33, 4, 8
    sig = planted(33, 150, n_hash, bands, rows)
    sig = np.vstack([sig, np.tile(sig[0], (70, 1))])
    n = len(sig)
    assert n == 220
    t = to_device(sig, n_hash + 5)
    index = device.lsh_index_build(t, n_hash, bands, rows)
    rows_of = np.arange(n, dtype=np.int32)
    for thr in (0.0, 0.5):
        i1, j1, c1 = (a.cpu().numpy() for a in device.lsh_edges(t, n_hash, bands, rows, thr))
        one = similarity.mh_lsh_last_route()
        i2, j2, c2 = (a.cpu().numpy() for a in device.lsh_cross_edges(index, t, t, n_hash, bands, rows, thr))
        two = similarity.mh_lsh_last_route()
        assert one["incidences"] >= bands * 71 * 70 // 2 and len(i1) > n
        off, up, low, diag = i1 != j1, i2 < j2, i2 > j2, i2 == j2
        assert (i1 <= j1).all() and off.sum() == up.sum() == low.sum() == len(i1) - n
        assert np.array_equal(i2[up], i1[off]) and np.array_equal(j2[up], j1[off]) and np.array_equal(c2[up], c1[off])
        order = np.lexsort((i2[low], j2[low]))                 # the lower triangle by (j, i): the upper one
        assert np.array_equal(j2[low][order], i1[off]) and np.array_equal(i2[low][order], j1[off]) and np.array_equal(c2[low][order], c1[off])
        assert np.array_equal(i2[diag], rows_of) and (c2[diag].view(np.uint16) == n_hash).all()
        assert two["incidences"] == 2 * one["incidences"] + n * bands and two["verified_pairs"] == 2 * one["verified_pairs"] + n
        idx1, key1 = (a.cpu().numpy() for a in device.lsh_knn(t, n_hash, bands, rows, 256, threshold=thr))
        idx2, key2 = (a.cpu().numpy() for a in device.lsh_cross_topk(index, t, t, n_hash, bands, rows, 257, threshold=thr))
        assert idx1.shape == key1.shape == (n, 256) and idx2.shape == key2.shape == (n, 257)
        others = idx2 != rows_of[:, None]                      # every row lists itself exactly once
        assert (others.sum(1) == 256).all() and (key2[~others].view(np.uint16) == n_hash).all()
        assert np.array_equal(idx2[others].reshape(n, 256), idx1) and np.array_equal(key2[others].reshape(n, 256), key1)
        assert (idx1 == -1).any() and (key1[idx1 == -1] == 0).all() and (idx1[:, :70] >= 0)[[0] + list(range(150, n))].all()


# ---- the pieces ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_hash,bands,rows", [(48, 12, 4), (33, 4, 8), (200, 3, 65), (31, 31, 1)])
def test_index_and_probe(da, n_hash, bands, rows):
    """for every (i, t): ids[lo : lo + len] are exactly the y rows whose band t equals x's band t, ascending; the index is sorted, is not
    changed by probing and does not depend on x"""
    from dynaalign_amd import device
    sig = planted(n_hash + 1, 170, n_hash, bands, rows)
    sig[5::11] = 0
    sig_x, sig_y = sig[:70], sig[70:]
    n = len(sig_y)
    tx, ty = to_device(sig_x, n_hash + 3), to_device(sig_y, n_hash + 6)
    index = device.lsh_index_build(ty, n_hash, bands, rows)
    assert index.dtype == torch.uint8 and index.numel() == device.lsh_index_bytes(n, bands)
    before = index.clone()
    lo, ln = device.lsh_index_probe(index, n, tx, n_hash, bands, rows)
    other = random_sig(5, 33, n_hash)
    other[:, :rows] = sig_y[:33, :rows]
    lo2, ln2 = device.lsh_index_probe(index, n, to_device(other), n_hash, bands, rows)
    torch.cuda.synchronize()
    assert torch.equal(index, before) and int(ln2[:, 0].min()) >= 1
    again = device.lsh_index_build(to_device(sig_y, n_hash), n_hash, bands, rows)           # another buffer, another leading dimension
    meta, band_start, keys, ids = (a.cpu().numpy() for a in device.lsh_index_arrays(index, n, bands))
    for a, b in zip(device.lsh_index_arrays(again, n, bands), (meta, band_start, keys, ids)):
        assert np.array_equal(a.cpu().numpy(), b)
    keys = keys.view(np.uint64)
    assert np.all(keys[1:] >= keys[:-1]) and band_start.tolist() == [t * n for t in range(bands + 1)]
    assert np.array_equal(keys >> np.uint64(48), np.repeat(np.arange(bands, dtype=np.uint64), n))
    runs = sum(len({tuple(r) for r in sig_y[:, t * rows:(t + 1) * rows].tolist()}) for t in range(bands))
    assert meta.view(np.uint32).tolist()[:5] == [0x4C534831, n, bands, rows, runs]
    lo, ln = lo.cpu().numpy(), ln.cpu().numpy()
    assert lo.shape == ln.shape == (70, bands) and ln.sum() > 0
    for i in range(70):
        for t in range(bands):
            same = np.flatnonzero((sig_y[:, t * rows:(t + 1) * rows] == sig_x[i, t * rows:(t + 1) * rows]).all(1))
            assert ids[lo[i, t]:lo[i, t] + ln[i, t]].tolist() == same.tolist(), (i, t)
            assert band_start[t] <= lo[i, t] <= band_start[t + 1]
    assert meta.view(np.uint32)[5] == np.unique(keys, return_counts=True)[1].max() >= ln.max()
    # an index built for other parameters is refused, not read
    with pytest.raises(da.DynaAlignError) as e:
        device.lsh_index_probe(index[:device.lsh_index_bytes(n - 1, bands)], n - 1, tx, n_hash, bands, rows)
    assert e.value.code == BAD_ARG and "not built for" in str(e.value)


def test_verify_pairs_on_triples_the_pipeline_would_not_produce(da):
    from dynaalign_amd import device
    n_hash, bands, rows = 48, 10, 4
    sig_x, sig_y = random_sig(5, 5, n_hash), random_sig(6, 7, n_hash)
    sig_y[0, 8:12] = sig_x[0, 8:12]                        # (0, 0): band 2 only
    sig_y[1, 4:8] = sig_x[1, 4:8]                          # (1, 1): bands 1 and 7
    sig_y[1, 28:32] = sig_x[1, 28:32]
    sig_y[2, 36:40] = sig_x[2, 36:40]                      # (2, 2): band 9 only, 4 / 48
    sig_y[3] = sig_x[3]                                    # (3, 3): every band
    sig_y[4, 8:11] = sig_x[4, 8:11]                        # (4, 4): band 2 but for its last column
    sig_y[4, 40:] = sig_x[4, 40:]
    tx, ty = to_device(sig_x, 64), to_device(sig_y, 52)
    triples = [(0, 0, 2), (0, 0, 1), (0, 0, 3), (0, 1, 0),      # its band; a key collision would name any other band: rejected
               (1, 1, 1), (1, 1, 7), (1, 1, 0),                 # first band kept, the later one rejected
               (2, 2, 9), (3, 3, 0), (3, 3, 9), (4, 4, 2),      # 3 of 4 columns: no agreement
               (0, 6, 0), (4, 6, 9),                            # j beyond m but inside n: read
               (5, 0, 0), (0, 7, 0), (-1, 1, 0), (0, -1, 0), (0, 0, 10), (0, 0, -1)]   # outside: nothing is read
    i, j, b = (np.array(v, np.int32) for v in zip(*triples))
    inside = lambda a, c, tb: 0 <= a < 5 and 0 <= c < 7 and 0 <= tb < bands
    want_count = [int((sig_x[a] == sig_y[c]).sum()) if inside(a, c, tb) else 0 for a, c, tb in triples]
    assert want_count[:11] == [4, 4, 4, 0, 8, 8, 8, 4, 48, 48, 11] and want_count[13:] == [0] * 6
    first = [True, False, False, False, True, False, False, True, True, False, False] + [False] * 8
    for thr, c_min in ((0.0, 0), (0.1, 5), (1.0, 48)):
        count, keep = device.lsh_cross_verify_pairs(tx, ty, n_hash, bands, rows, thr, i, j, b)
        torch.cuda.synchronize()
        assert count.cpu().numpy().view(np.uint16).tolist() == want_count      # the count comes back for rejected triples too
        assert keep.cpu().tolist() == [int(f and c >= c_min) for f, c in zip(first, want_count)], thr
    # more triples than one chunk of 64, and a number that is no multiple of it; given as CPU tensors that are not int32
    many = [(a, c, tb) for a in range(5) for c in range(7) for tb in range(bands)][:257]
    i, j, b = (torch.tensor(v, dtype=torch.int64) for v in zip(*many))
    count, keep = device.lsh_cross_verify_pairs(tx, ty, n_hash, bands, rows, 0.05, i, j, b)
    agree = lambda a, c, tb: bool((sig_x[a, tb * 4:tb * 4 + 4] == sig_y[c, tb * 4:tb * 4 + 4]).all())
    want_keep = [int(agree(a, c, tb) and not any(agree(a, c, u) for u in range(tb)) and (sig_x[a] == sig_y[c]).sum() / 48 >= 0.05) for a, c, tb in many]
    assert keep.is_cuda and keep.cpu().tolist() == want_keep and sum(want_keep) == 4
    assert count.cpu().numpy().view(np.uint16).tolist() == [int((sig_x[a] == sig_y[c]).sum()) for a, c, _ in many]


# ---- caps, workspace and route ------------------------------------------------------------------------------------------------------------
def test_capacity_and_the_cap(da):
    from dynaalign_amd import device, similarity
    row = random_sig(4, 1, 31)
    sig_x, sig_y = np.tile(row, (6, 1)), np.vstack([np.tile(row, (20, 1)), random_sig(5, 4, 31)])
    want = cross_model(sig_x, sig_y, 5, 6, 0.5)
    assert want["incidences"] == 5 * 6 * 20 and want["largest"] == 20 and len(want["i"]) == 120
    tx, ty = to_device(sig_x, 32), to_device(sig_y, 40)
    index = device.lsh_index_build(ty, 31, 5, 6)
    i, j, c = device.lsh_cross_edges(index, tx, ty, 31, 5, 6, 0.5, capacity=7)
    assert (i.cpu().tolist(), j.cpu().tolist()) == (want["i"][:7], want["j"][:7]) and similarity.mh_lsh_last_route()["edges"] == 120
    i, j, c = device.lsh_cross_edges(index, tx, ty, 31, 5, 6, 0.5, capacity=120, max_candidates=600)     # exactly the counts pass
    same_cross_edges((i.cpu().numpy(), j.cpu().numpy(), weights(c, 31)), want)
    idx, key = device.lsh_cross_topk(index, tx, ty, 31, 5, 6, 3, max_candidates=600)
    assert idx.cpu().tolist() == [[0, 1, 2]] * 6
    for call in (lambda: device.lsh_cross_edges(index, tx, ty, 31, 5, 6, 0.5, max_candidates=599),
                 lambda: device.lsh_cross_topk(index, tx, ty, 31, 5, 6, 3, max_candidates=599)):
        with pytest.raises(da.DynaAlignError) as e:
            call()
        assert e.value.code == UNSUPPORTED
        assert "600 (pair, band) candidates" in str(e.value) and "max_candidates = 599" in str(e.value) and "largest bucket: 20" in str(e.value)
    # the host entry refuses likewise
    x, y = ["ACDEFGHIKLMNPQRSTVWY"] * 6, ["ACDEFGHIKLMNPQRSTVWY"] * 20 + ["WWWWWYYYYYWWWWWYYYYY"]
    assert len(da.similarityMH_lsh_cross_edges(x, y, 4, 48, 12, 4, 0.5, seed=SEED, max_candidates=12 * 120)[1]) == 120
    with pytest.raises(da.DynaAlignError) as e:
        da.similarityMH_lsh_cross_edges(x, y, 4, 48, 12, 4, 0.5, seed=SEED, max_candidates=12 * 120 - 1)
    assert e.value.code == UNSUPPORTED and "1440" in str(e.value) and "max_candidates = 1439" in str(e.value) and "largest bucket: 20" in str(e.value)


def test_workspace_of_any_alignment_and_a_host_workspace(da):
    from dynaalign_amd import device
    sig = planted(11, 150, 48, 12, 4)
    sig_x, sig_y = sig[:60], sig[60:]
    want = cross_model(sig_x, sig_y, 12, 4, 0.5)
    tx, ty = to_device(sig_x, 64), to_device(sig_y, 56)
    index = device.lsh_index_build(ty, 48, 12, 4)
    need = device.lsh_cross_workspace_bytes(60, 12)
    big = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    off = (-big.data_ptr()) % 256 + 4
    work = big[off:off + need]
    assert work.data_ptr() % 256 == 4
    i, j, c = device.lsh_cross_edges(index, tx, ty, 48, 12, 4, 0.5, work=work)
    torch.cuda.synchronize()
    same_cross_edges((i.cpu().numpy(), j.cpu().numpy(), weights(c, 48)), want)
    idx, key = device.lsh_cross_topk(index, tx, ty, 48, 12, 4, 5, threshold=0.5, work=work)
    same_cross_lists((idx.cpu().numpy(), weights(key, 48)), *topk_model(want, 60, 5))
    for bad in (torch.empty(need, dtype=torch.uint8), big[:need - 1]):                     # on the host; one byte short
        with pytest.raises(da.DynaAlignError):
            device.lsh_cross_edges(index, tx, ty, 48, 12, 4, 0.5, work=bad)
    with pytest.raises(da.DynaAlignError):
        device.lsh_cross_edges(index.cpu(), tx, ty, 48, 12, 4, 0.5)


# ---- the session --------------------------------------------------------------------------------------------------------------------------
def csr_to_edges(got):
    thr, rowptr, j, w = got
    assert rowptr.is_cuda and rowptr.dtype == torch.int64 and j.dtype == torch.int32 and w.dtype == torch.float64
    rp = rowptr.cpu().numpy()
    assert rp[0] == 0 and rp[-1] == j.numel() == w.numel() and np.all(np.diff(rp) >= 0)
    return thr, np.repeat(np.arange(len(rp) - 1, dtype=np.int32), np.diff(rp)), j.cpu().numpy(), w.cpu().numpy()


def test_session_queries_a_kept_index(da):
    from dynaalign_amd import session
    seqs = family(1, 6, 20, 300) + FIXED
    s = session.MinHashSession(seqs, 4, 48, seed=SEED, reserve=False)
    batches = [family(1, 6, 20, 90)[40:] + FIXED, family(7, 6, 20, 30) + seqs[10:25]]
    idx = np.random.RandomState(9).permutation(len(seqs))[:173]
    index = s.lsh_index(12, 4)
    assert s.lsh_index(12, 4) is index and s.lsh_index(12, 4, idx) is not index and s.lsh_index(12, 4, idx) is s.lsh_index(12, 4, idx.copy())
    kept = index.clone()
    for resident, ix in ((seqs, None), ([seqs[t] for t in idx], idx)):
        for new in batches:
            want = da.similarityMH_lsh_cross_edges(new, resident, 4, 48, 12, 4, 0.5, seed=s.seed)
            assert len(want[1]) > 0
            got = csr_to_edges(s.lsh_cross_edges(new, 12, 4, 0.5, idx=ix))
            assert got[0] == want[0] == 0.5
            for a, b in zip(got[1:], want[1:]):
                assert a.dtype == b.dtype and np.array_equal(a, b)
            assert np.array_equal(got[3].view(np.uint64), want[3].view(np.uint64))
            for top in (3, 400):                               # 400: more than the subset has rows -- not clamped
                wi, wv = da.similarityMH_lsh_cross_topk(new, resident, 4, 48, 12, 4, top, threshold=0.3, seed=s.seed)
                gi, gv = s.lsh_cross_topk(new, 12, 4, top, idx=ix, threshold=0.3)
                assert gi.dtype == np.int32 and gi.shape == (len(new), top) and np.array_equal(gi, wi)
                assert np.array_equal(gv.view(np.uint64), wv.view(np.uint64))
    assert s.lsh_index(12, 4) is index and torch.equal(index, kept)      # neither rebuilt nor written by the queries
    with pytest.raises(da.DynaAlignError) as e:
        s.lsh_cross_edges(batches[0], 12, 4, 0.5, max_candidates=10)
    assert e.value.code == UNSUPPORTED


def test_one_row_bands_give_the_lists_of_cross_topk(da):
    from dynaalign_amd import session
    seqs = family(2, 5, 20, 200) + FIXED
    new = family(2, 5, 20, 260)[200:] + ["WWWWWYYYYYWWWWWYYYYY", ""]
    s = session.MinHashSession(seqs, 2, 50, seed=SEED, reserve=False)
    ci, cv = s.cross_topk(new, 10)
    li, lv = s.lsh_cross_topk(new, 50, 1, 10)
    real = cv > 0
    assert real.any() and not real.all()
    assert np.array_equal(li[real], ci[real]) and np.array_equal(lv[real].view(np.uint64), cv[real].view(np.uint64))
    assert (li[~real] == -1).all() and (lv[~real] == 0.0).all()
