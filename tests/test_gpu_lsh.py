"""GPU tests of MinHash LSH banding (lsh_kernels.hip): similarityMH_lsh_edges, the device pieces (da_dev_lsh_band_keys / _verify_pairs /
_edges), MinHashSession.lsh_edges and clusterbreak on the LSH graph.  Every comparison is exact -- indices as integers, weights as uint64
bit patterns -- against this file's own model (test_lsh_cpu.model: dicts from a band's values to its members, a Python count) on the
oracle's signatures or on synthetic signature tensors."""
import numpy as np
import pytest
import torch

import oracle_lib as O
from test_gpu_jaccard import family
from test_lsh_cpu import FIXED, model, same_edges

pytestmark = pytest.mark.gpu

SEED = 12345
UNSUPPORTED = 10
# (k, n_hash, bands, rows, threshold) -> (seed, parents, length, count) of family(); the five fixed strings follow
CASES = [((4, 48, 12, 4, 0.5), (1, 6, 20, 300)), ((2, 50, 10, 5, 0.6), (2, 5, 20, 257)), ((3, 100, 33, 3, 0.4), (3, 8, 24, 300)),
         ((4, 64, 1, 64, 0.3), (4, 6, 20, 300)), ((4, 40, 40, 1, 0.5), (5, 6, 20, 300))]


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    from dynaalign_amd import _capi
    assert _capi.load().da_device_count() > 0
    return dynaalign_amd


def oracle_sig(seqs, k, n_hash):
    return O.signatures(seqs, k, n_hash, O.seeds(SEED, n_hash))


def all_pairs_edges(sig, threshold):
    """the strict upper triangle of the all-pairs threshold graph, as a set of (i, j)"""
    s = O.mh_counts(sig).astype(np.float64) / np.float64(sig.shape[1])
    i, j = np.nonzero(np.triu((s >= threshold) & (s > 0), 1))
    return set(zip(i.tolist(), j.tolist()))


@pytest.mark.parametrize("params,fam", CASES, ids=["12x4", "10x5", "33x3", "1x64", "40x1"])
def test_host_entry_equals_the_model_on_oracle_signatures(da, params, fam):
    from dynaalign_amd import similarity
    k, n_hash, bands, rows, thr = params
    seqs = family(*fam) + FIXED
    sig = oracle_sig(seqs, k, n_hash)
    want = model(sig, bands, rows, thr)
    # what the inputs were chosen for
    assert want["incidences"] > 0 and len(want["i"]) > len(seqs)
    must_not_add = all_pairs_edges(sig, thr) - want["pairs"]
    if bands > 1:
        assert want["multi"] > 0 and want["below"] > 0
    if rows > 1:
        assert len(must_not_add) > 0
    if rows == 1:
        assert want["largest"] > 32
    got_thr, i, j, w = da.similarityMH_lsh_edges(seqs, k, n_hash, bands, rows, thr, seed=SEED)
    assert got_thr == thr
    same_edges((i, j, w), want)
    assert not (set(zip(i.tolist(), j.tolist())) & must_not_add)
    route = similarity.mh_lsh_last_route()
    assert route["incidences"] == want["incidences"] and route["verified_pairs"] == len(want["pairs"]) and route["edges"] == len(i)
    assert route["buckets"] == sum(len({tuple(r) for r in sig[:, t * rows:(t + 1) * rows].tolist()}) for t in range(bands))
    # the numpy definition agrees as well
    same_edges(da.lsh_edges_dense(da.minhash_signatures(seqs, k, n_hash, seed=SEED), bands, rows, thr), want)


def test_one_and_two_sequences(da):
    thr, i, j, w = da.similarityMH_lsh_edges(["ACDEFGHIK"], 4, 8, 2, 4, 0.5, seed=SEED)
    assert (i.tolist(), j.tolist(), w.tolist()) == ([0], [0], [1.0])
    thr, i, j, w = da.similarityMH_lsh_edges([""], 4, 8, 2, 4, 0.5, seed=SEED, max_candidates=0)
    assert (i.tolist(), j.tolist(), w.tolist()) == ([0], [0], [1.0])
    for two in (["ACDEFGHIK", "ACDEFGHIK"], ["ACDEFGHIK", "WWWWWYYYYY"], ["ACDEFGHIKLMNPQRSTVWY", "ACDEFGHIKLMNPQRSTVWW"]):
        want = model(oracle_sig(two, 4, 48), 12, 4, 0.5)
        _, i, j, w = da.similarityMH_lsh_edges(two, 4, 48, 12, 4, 0.5, seed=SEED)
        same_edges((i, j, w), want)
    assert len(i) == 3                                       # the near duplicate is an edge


@pytest.fixture(scope="module")
def with_copies():
    """the first set with 300 byte-identical copies appended: a bucket larger than a wave and than a workgroup in every band"""
    seqs = family(1, 6, 20, 300) + FIXED + ["ACDEFGHIKLMNPQRSTVWA"] * 300
    sig = oracle_sig(seqs, 4, 48)
    return seqs, model(sig, 12, 4, 0.5)


def test_a_bucket_larger_than_a_workgroup(da, with_copies):
    seqs, want = with_copies
    assert want["largest"] >= 300 and want["incidences"] >= 12 * 44850
    w_all = np.array(want["w"])
    assert int(((np.array(want["i"]) >= 305) & (np.array(want["j"]) > np.array(want["i"])) & (w_all == 1.0)).sum()) == 44850
    _, i, j, w = da.similarityMH_lsh_edges(seqs, 4, 48, 12, 4, 0.5, seed=SEED)
    same_edges((i, j, w), want)


def test_more_candidates_than_the_cap_is_refused_with_the_count(da, with_copies):
    seqs, want = with_copies
    with pytest.raises(da.DynaAlignError) as e:
        da.similarityMH_lsh_edges(seqs, 4, 48, 12, 4, 0.5, seed=SEED, max_candidates=1000)
    assert e.value.code == UNSUPPORTED
    text = str(e.value)
    assert str(want["incidences"]) in text and "max_candidates = 1000" in text and "largest bucket: %d" % want["largest"] in text
    # exactly the count is enough
    _, i, _, _ = da.similarityMH_lsh_edges(seqs, 4, 48, 12, 4, 0.5, seed=SEED, max_candidates=want["incidences"])
    assert len(i) == len(want["i"])
    with pytest.raises(da.DynaAlignError):
        da.similarityMH_lsh_edges(seqs, 4, 48, 12, 4, 0.5, seed=SEED, max_candidates=want["incidences"] - 1)


# ---- the device pieces on synthetic signatures ------------------------------------------------------------------------------------------
def to_device(sig, ld=None, pad=0x5A5A5A5A):
    """(n, n_hash) uint32 -> an int32 tensor view (n, n_hash) of a buffer of leading dimension ld whose padding columns hold one equal value"""
    n, n_hash = sig.shape
    ld = n_hash if ld is None else ld
    buf = np.full((n, ld), pad, np.uint32)
    buf[:, :n_hash] = sig
    return torch.from_numpy(buf.view(np.int32)).cuda()[:, :n_hash]


def device_edges(da, sig, bands, rows, thr, ld=None, **kw):
    from dynaalign_amd import device
    t = to_device(sig, ld)
    i, j, c = device.lsh_edges(t, sig.shape[1], bands, rows, thr, **kw)
    torch.cuda.synchronize()
    c = c.cpu().numpy().view(np.uint16)
    return i.cpu().numpy(), j.cpu().numpy(), c.astype(np.float64) / np.float64(sig.shape[1])


def random_sig(seed, n, n_hash):
    return np.random.RandomState(seed).randint(0, 1 << 32, (n, n_hash), dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("n_hash,bands,rows", [(1, 1, 1), (31, 5, 6), (31, 31, 1), (33, 1, 33), (33, 4, 8), (48, 12, 4), (48, 2, 17), (200, 3, 65),
                                               (600, 9, 64)])
def test_device_edges_on_planted_signatures(da, n_hash, bands, rows):
    """random signatures with planted agreements (whole rows, first / last / two bands, a band but for its last column, the tail columns
    only), values 0 and 0xFFFFFFFF among them, in a buffer with ld_sig > n_hash whose padding is equal in all rows"""
    from test_lsh_cpu import planted
    sig = planted(n_hash, 150, n_hash, bands, rows)
    sig[::7, ::3] = 0
    sig[3::11] = 0xFFFFFFFF
    sig[5::11] = 0
    for thr in (0.0, 0.5, 1.0):
        want = model(sig, bands, rows, thr)
        assert want["incidences"] > 0
        same_edges(device_edges(da, sig, bands, rows, thr, ld=n_hash + 5), want)


def test_all_rows_equal_and_all_rows_distinct(da):
    eq = np.tile(random_sig(1, 1, 48), (130, 1))
    want = model(eq, 12, 4, 0.5)
    assert len(want["i"]) == 130 * 131 // 2 and set(want["w"]) == {1.0}
    same_edges(device_edges(da, eq, 12, 4, 0.5, ld=64), want)
    distinct = random_sig(2, 130, 48)
    want = model(distinct, 12, 4, 0.0)
    assert want["incidences"] == 0 and len(want["i"]) == 130
    same_edges(device_edges(da, distinct, 12, 4, 0.0), want)
    for value in (0, 0xFFFFFFFF):
        const = np.full((70, 33), value, np.uint32)
        same_edges(device_edges(da, const, 4, 8, 1.0, ld=40), model(const, 4, 8, 1.0))


def test_tail_columns_count_but_make_no_candidate_and_bands_dedup(da):
    from dynaalign_amd import similarity
    n_hash, bands, rows = 48, 10, 4                        # columns 40 .. 47 belong to no band
    sig = random_sig(3, 8, n_hash)
    sig[1, 40:] = sig[0, 40:]                              # agreement in the tail only: no candidate
    sig[3, 36:40] = sig[2, 36:40]                          # the last band only
    sig[5, 0:4] = sig[4, 0:4]                              # band 0 and the last band: one edge
    sig[5, 36:40] = sig[4, 36:40]
    sig[7, 0:4] = sig[6, 0:4]                              # a candidate whose tail counts towards the threshold
    sig[7, 40:] = sig[6, 40:]
    want = model(sig, bands, rows, 0.0)
    assert (0, 1) not in want["pairs"] and want["bands_of"][(2, 3)] == [9] and want["bands_of"][(4, 5)] == [0, 9]
    i, j, w = device_edges(da, sig, bands, rows, 0.0, ld=64)
    same_edges((i, j, w), want)
    route = similarity.mh_lsh_last_route()
    assert route["incidences"] == 4 and route["verified_pairs"] == 3 and route["edges"] == 8 + 3
    pairs = list(zip(i.tolist(), j.tolist(), w.tolist()))
    assert (2, 3, 4 / 48) in pairs and (4, 5, 8 / 48) in pairs and (6, 7, 12 / 48) in pairs
    # the threshold is applied to the whole count: 12 / 48 passes 0.25, 8 / 48 does not
    same_edges(device_edges(da, sig, bands, rows, 0.25), model(sig, bands, rows, 0.25))
    assert len(model(sig, bands, rows, 0.25)["i"]) == 8 + 1


def test_capacity_and_the_cap_on_the_device_entry(da):
    from dynaalign_amd import device, similarity
    sig = np.tile(random_sig(4, 1, 31), (20, 1))
    want = model(sig, 5, 6, 0.5)
    t = to_device(sig, 32)
    i, j, c = device.lsh_edges(t, 31, 5, 6, 0.5, capacity=7)
    assert (i.cpu().tolist(), j.cpu().tolist()) == (want["i"][:7], want["j"][:7]) and similarity.mh_lsh_last_route()["edges"] == len(want["i"])
    with pytest.raises(da.DynaAlignError) as e:
        device.lsh_edges(t, 31, 5, 6, 0.5, max_candidates=5 * 190 - 1)
    assert e.value.code == UNSUPPORTED and "950" in str(e.value) and "largest bucket: 20" in str(e.value)


def test_workspace_of_any_alignment_and_host_side_triples(da):
    """a caller's workspace that starts 4 bytes off a 256-byte boundary; triples given as CPU tensors are moved to the device, a CPU
    workspace is refused before anything is launched"""
    from dynaalign_amd import device
    from test_lsh_cpu import planted
    sig = planted(11, 150, 48, 12, 4)
    want = model(sig, 12, 4, 0.5)
    t = to_device(sig, 64)
    big = torch.empty(device.lsh_workspace_bytes(150, 12) + 256, dtype=torch.uint8, device="cuda")
    off = (-big.data_ptr()) % 256 + 4
    work = big[off:off + device.lsh_workspace_bytes(150, 12)]
    assert work.data_ptr() % 256 == 4
    i, j, c = device.lsh_edges(t, 48, 12, 4, 0.5, work=work)
    torch.cuda.synchronize()
    same_edges((i.cpu().numpy(), j.cpu().numpy(), c.cpu().numpy().view(np.uint16).astype(np.float64) / np.float64(48)), want)
    with pytest.raises(da.DynaAlignError):
        device.lsh_edges(t, 48, 12, 4, 0.5, work=torch.empty(device.lsh_workspace_bytes(150, 12), dtype=torch.uint8))
    pairs = sorted(want["bands_of"])[:70]
    ti = torch.tensor([p[0] for p in pairs], dtype=torch.int64)               # on the host, and not int32
    tj = torch.tensor([p[1] for p in pairs], dtype=torch.int64)
    tb = torch.tensor([want["bands_of"][p][0] for p in pairs], dtype=torch.int64)
    count, keep = device.lsh_verify_pairs(t, 48, 12, 4, 0.0, ti, tj, tb)
    assert keep.is_cuda and keep.cpu().tolist() == [1] * len(pairs)
    assert count.cpu().numpy().view(np.uint16).tolist() == [int((sig[a] == sig[b]).sum()) for a, b in pairs]


@pytest.mark.parametrize("n_hash,bands,rows", [(48, 12, 4), (33, 4, 8), (200, 3, 65)])
def test_band_keys(da, n_hash, bands, rows):
    """equal band values <-> equal keys, the band number on top, ids = the row; the padding and the columns behind the last band are not read"""
    from dynaalign_amd import device
    from test_lsh_cpu import planted
    sig = planted(7, 90, n_hash, bands, rows)
    keys, ids = device.lsh_band_keys(to_device(sig, n_hash + 3), n_hash, bands, rows)
    other = sig.copy()
    other[:, bands * rows:] ^= 0xFFFF
    keys2, _ = device.lsh_band_keys(to_device(other, n_hash + 7, pad=7), n_hash, bands, rows)
    torch.cuda.synchronize()
    keys, ids = keys.cpu().numpy().view(np.uint64), ids.cpu().numpy()
    assert np.array_equal(keys, keys2.cpu().numpy().view(np.uint64))
    assert np.array_equal(ids, np.repeat(np.arange(90, dtype=np.int32)[:, None], bands, 1))
    assert np.array_equal(keys >> np.uint64(48), np.repeat(np.arange(bands, dtype=np.uint64)[None, :], 90, 0))
    for t in range(bands):
        values = [tuple(r) for r in sig[:, t * rows:(t + 1) * rows].tolist()]
        by_value, by_key = {}, {}
        for r in range(90):
            by_value.setdefault(values[r], []).append(r)
            by_key.setdefault(int(keys[r, t]), []).append(r)
        assert sorted(by_value.values()) == sorted(by_key.values())


def test_verify_pairs_on_triples_the_pipeline_would_not_produce(da):
    from dynaalign_amd import device
    n_hash, bands, rows = 48, 10, 4
    sig = random_sig(5, 10, n_hash)
    sig[1, 8:12] = sig[0, 8:12]                            # (0, 1): band 2 only
    sig[3, 4:8] = sig[2, 4:8]                              # (2, 3): bands 1 and 7
    sig[3, 28:32] = sig[2, 28:32]
    sig[5, 36:40] = sig[4, 36:40]                          # (4, 5): band 9 only, 4 / 48
    sig[7] = sig[6]                                        # (6, 7): every band
    sig[9, 8:11] = sig[8, 8:11]                            # (8, 9): band 2 but for its last column
    sig[9, 40:] = sig[8, 40:]
    t = to_device(sig, 64)
    triples = [(0, 1, 2), (0, 1, 1), (0, 1, 3), (0, 2, 0),      # its band; a key collision would name any other band: rejected
               (2, 3, 1), (2, 3, 7), (2, 3, 0),                 # first band kept, the later one rejected
               (4, 5, 9), (6, 7, 0), (6, 7, 9), (7, 6, 0),      # (7, 6): the decision is symmetric
               (8, 9, 2), (3, 3, 0),                            # 3 of 4 columns: no agreement; a row with itself
               (0, 10, 0), (-1, 1, 0), (0, 1, 10), (0, 1, -1)]  # outside: nothing is read
    i, j, b = (np.array(x, np.int32) for x in zip(*triples))
    for thr, c_min in ((0.0, 0), (0.1, 5), (1.0, 48)):
        count, keep = device.lsh_verify_pairs(t, n_hash, bands, rows, thr, i, j, b)
        torch.cuda.synchronize()
        count, keep = count.cpu().numpy().view(np.uint16).tolist(), keep.cpu().tolist()
        want_count = [int((sig[a] == sig[c]).sum()) if 0 <= a < 10 and 0 <= c < 10 and 0 <= tb < bands else 0 for a, c, tb in triples]
        assert want_count[:13] == [4, 4, 4, 0, 8, 8, 8, 4, 48, 48, 48, 11, 48]
        first = [True, False, False, False, True, False, False, True, True, False, True, False, True, False, False, False, False]
        assert count == want_count                             # the count comes back for rejected triples too
        assert keep == [int(f and c >= c_min) for f, c in zip(first, want_count)], thr
    # more triples than one chunk of 64, and a number that is no multiple of it
    many = [(a, c, tb) for a in range(10) for c in range(10) for tb in (0, 2, 9)][:257]
    i, j, b = (np.array(x, np.int32) for x in zip(*many))
    count, keep = device.lsh_verify_pairs(t, n_hash, bands, rows, 0.05, i, j, b)
    agree = lambda a, c, tb: bool((sig[a, tb * 4:tb * 4 + 4] == sig[c, tb * 4:tb * 4 + 4]).all())
    want_keep = [int(agree(a, c, tb) and not any(agree(a, c, u) for u in range(tb)) and (sig[a] == sig[c]).sum() / 48 >= 0.05) for a, c, tb in many]
    assert keep.cpu().tolist() == want_keep and sum(want_keep) > 10
    assert count.cpu().numpy().view(np.uint16).tolist() == [int((sig[a] == sig[c]).sum()) for a, c, _ in many]


# ---- session and clusterbreak -----------------------------------------------------------------------------------------------------------
def test_session_equals_the_host_call_on_a_subset(da):
    from dynaalign_amd import session
    seqs = family(1, 6, 20, 300) + FIXED
    s = session.MinHashSession(seqs, 4, 48, seed=SEED, reserve=False)
    idx = np.random.RandomState(9).permutation(len(seqs))[:173]
    for sub, ix in ((seqs, None), ([seqs[t] for t in idx], idx)):
        want = da.similarityMH_lsh_edges(sub, 4, 48, 12, 4, 0.5, seed=s.seed)
        got = s.lsh_edges(12, 4, 0.5, idx=ix)
        assert got[0] == want[0] == 0.5 and len(want[1]) > len(sub)
        for a, b in zip(got[1:], want[1:]):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        assert np.array_equal(got[3].view(np.uint64), want[3].view(np.uint64))
    with pytest.raises(da.DynaAlignError) as e:
        s.lsh_edges(12, 4, 0.5, max_candidates=10)
    assert e.value.code == UNSUPPORTED


def test_clusterbreak_on_the_lsh_graph(da):
    pep = family(1, 6, 20, 300)

    def dense_fn(sub):
        i, j, w = da.lsh_edges_dense(oracle_sig(sub, 4, 48), 12, 4, 0.5)
        return 0.5, i, j, w
    a = da.clusterbreak(pep, size_max=40, edges_fn=lambda s: da.similarityMH_lsh_edges(s, 4, 48, 12, 4, 0.5, seed=SEED))
    b = da.clusterbreak(pep, size_max=40, edges_fn=dense_fn)
    assert np.array_equal(a["clustered_seq"], b["clustered_seq"]) and a["filtered_seq"] == b["filtered_seq"]
    assert a.calls == b.calls >= 1 and [l["edges"] for l in a.levels] == [l["edges"] for l in b.levels]
