"""GPU tests of the LSH nearest-neighbour lists (lsh_kernels.hip: k_lsh_knn_entries, k_lsh_knn_select_short / _long): the selection on
synthetic ragged rows, da_dev_lsh_knn on synthetic signatures, the host entry, MinHashSession.lsh_knn / lsh_knn_csr and clusterbreak's
knn_lsh.  Every comparison is exact -- indices as integers, values as uint64 bit patterns -- against numpy sorts of the rows, closed forms,
or the Python model of test_lsh_knn_cpu on the oracle's signatures."""
import numpy as np
import pytest
import torch

import oracle_lib as O
from test_gpu_jaccard import family
from test_gpu_lsh import CASES, SEED, oracle_sig, random_sig, to_device
from test_lsh_cpu import FIXED, model, planted
from test_lsh_knn_cpu import knn_model, same_lists

pytestmark = pytest.mark.gpu

UNSUPPORTED = 10


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    from dynaalign_amd import _capi
    assert _capi.load().da_device_count() > 0
    return dynaalign_amd


# ---- the selection on synthetic ragged rows -----------------------------------------------------------------------------------------------
def degrees_for(top):
    """0, 1, around top, around a wave, one below / at / above both class boundaries of the kernel, and two long rows"""
    from dynaalign_amd import device
    w, b = device.LSH_KNN_WAVE_MAX, device.LSH_KNN_LDS_WORDS
    assert (w, b) == (64, 2048)
    return [0, 1, max(top - 1, 0), top, top + 1, 63, 64, 65, w - 1, w, w + 1, 0, b - 1, b, b + 1, 5000, 70000, 3]


def ragged_rows(degrees, pattern, top, seed):
    """-> (ptr int64, col int32, count uint16): distinct columns from the whole non-negative int32 range in random order, 2^31 - 1 and 0 among
    them; counts by pattern"""
    rng = np.random.RandomState(seed)
    ptr = np.zeros(len(degrees) + 1, np.int64)
    ptr[1:] = np.cumsum(degrees)
    cols, counts = [], []
    for deg in degrees:
        c = rng.permutation(np.unique(rng.randint(1, (1 << 31) - 1, deg + 64, dtype=np.int64)))[:deg]
        if deg >= 2:                                                   # both ends of the range: every digit of a column is exercised
            c[:2] = 0, (1 << 31) - 1
            c = rng.permutation(c)
        assert len(set(c.tolist())) == deg
        if pattern == "equal":                                         # the column digits alone decide
            v = np.full(deg, 7, np.int64)
        elif pattern == "straddle":                                    # top - 1 (or half the row) at the high value: position top falls among the low ones
            v = np.full(deg, 299, np.int64)
            v[rng.permutation(deg)[:(top - 1 if deg > top else deg // 2)]] = 300
        elif pattern == "extremes":
            v = rng.choice(np.array([0, 65535, 1000, 256, 255], np.int64), deg)
        else:
            v = rng.randint(0, 65536, deg).astype(np.int64)
        cols.append(c)
        counts.append(v)
    return ptr, np.concatenate(cols).astype(np.int32), np.concatenate(counts).astype(np.uint16)


def select_reference(ptr, col, count, top, nnz=None):
    """per row: a numpy sort by (count descending, column ascending) of the entries inside [0, nnz), the first top, then -1 / 0"""
    nnz = len(col) if nnz is None else nnz
    n = len(ptr) - 1
    idx = np.full((n, top), -1, np.int32)
    key = np.zeros((n, top), np.uint16)
    for r in range(n):
        b, e = min(max(int(ptr[r]), 0), nnz), min(max(int(ptr[r + 1]), 0), nnz)
        e = max(e, b)
        c, v = col[b:e].astype(np.int64), count[b:e].astype(np.int64)
        order = np.lexsort((c, -v))[:top]
        idx[r, :len(order)] = c[order]
        key[r, :len(order)] = v[order]
    return idx, key


def run_select(ptr, col, count, top, nnz=None, pad=3):
    from dynaalign_amd import device
    n = len(ptr) - 1
    out_i = torch.full((n, top + pad), 77, dtype=torch.int32, device="cuda")
    out_k = torch.full((n, top + pad), 77, dtype=torch.int16, device="cuda")
    t_ptr, t_col = torch.from_numpy(ptr).cuda(), torch.from_numpy(col).cuda()
    t_cnt = torch.from_numpy(count.view(np.int16)).cuda()
    idx, key = device.lsh_knn_select(t_ptr, t_col, t_cnt, top, nnz=nnz, out=(out_i, out_k))
    torch.cuda.synchronize()
    assert idx.shape == (n, top) and key.shape == (n, top)
    assert (out_i[:, top:] == 77).all() and (out_k[:, top:] == 77).all()          # the padding columns of the outputs are untouched
    return idx.cpu().numpy(), key.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("top", [1, 10, 64, 1000, 1024])
def test_select_on_synthetic_ragged_rows(da, top):
    for p, pattern in enumerate(("equal", "straddle", "extremes", "random")):
        ptr, col, count = ragged_rows(degrees_for(top), pattern, top, 100 * top + p)
        assert col.max() == (1 << 31) - 1 and col.min() == 0
        want_i, want_k = select_reference(ptr, col, count, top)
        got_i, got_k = run_select(ptr, col, count, top)
        assert np.array_equal(got_i, want_i), pattern
        assert np.array_equal(got_k, want_k), pattern
        assert np.array_equal(got_i >= 0, np.arange(top)[None, :] < np.minimum(np.diff(ptr), top)[:, None])


def test_select_without_workspace_outputs_and_refusals(da):
    from dynaalign_amd import device
    ptr, col, count = ragged_rows([5, 0, 70, 3000], "random", 4, 5)
    t = [torch.from_numpy(a).cuda() for a in (ptr, col, count.view(np.int16))]
    idx, key = device.lsh_knn_select(*t, 4)                               # outputs allocated by the call, ld = top
    torch.cuda.synchronize()
    want_i, want_k = select_reference(ptr, col, count, 4)
    assert np.array_equal(idx.cpu().numpy(), want_i) and np.array_equal(key.cpu().numpy().view(np.uint16), want_k)
    for bad_top in (0, 1025):
        with pytest.raises(da.DynaAlignError) as e:
            device.lsh_knn_select(*t, bad_top)
        assert str(e.value) == "top must be in 1 .. 1024 (got %d)" % bad_top
    with pytest.raises(da.DynaAlignError):
        device.lsh_knn_select(t[0].cpu(), t[1], t[2], 4)                  # a host tensor is refused before anything is launched


def test_select_cuts_rows_to_the_entries_inside_nnz(da):
    """a clamp on valid memory: col / count are allocated at full length, a smaller nnz is passed, and one row's pointer runs backwards"""
    degrees = [3, 70, 10, 3000, 40, 5, 100]
    ptr, col, count = ragged_rows(degrees, "random", 10, 6)
    nnz = int(ptr[3]) + 1500                                              # inside row 3: rows 4 .. 6 lie behind it
    for top in (10, 1024):
        want_i, want_k = select_reference(ptr, col, count, top, nnz)
        assert (want_i[3] >= 0).sum() == min(1500, top) and (want_i[4:] == -1).all()
        got_i, got_k = run_select(ptr, col, count, top, nnz=nnz)
        assert np.array_equal(got_i, want_i) and np.array_equal(got_k, want_k)
    back = ptr.copy()
    back[2] = ptr[1] - 2                                                  # row 1 runs backwards (empty), row 2 then starts inside row 0
    want_i, want_k = select_reference(back, col, count, 10)
    assert (want_i[1] == -1).all() and (want_i[2] >= 0).all()
    got_i, got_k = run_select(back, col, count, 10)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_k, want_k)


# ---- the whole pipeline on synthetic signatures ---------------------------------------------------------------------------------------------
def device_lists(sig, bands, rows, top, thr=0.0, ld=None, **kw):
    from dynaalign_amd import device
    idx, key = device.lsh_knn(to_device(sig, ld), sig.shape[1], bands, rows, top, threshold=thr, **kw)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), key.cpu().numpy().view(np.uint16).astype(np.float64) / np.float64(sig.shape[1])


@pytest.mark.parametrize("n_hash,bands,rows", [(31, 5, 6), (33, 4, 8), (48, 12, 4), (200, 3, 65)])
def test_device_lists_on_planted_signatures(da, n_hash, bands, rows):
    from dynaalign_amd import similarity
    sig = planted(n_hash, 150, n_hash, bands, rows)
    sig[::7, ::3] = 0
    sig[3::11] = 0xFFFFFFFF
    sig[5::11] = 0
    for thr in (0.0, 0.5):
        full_i, full_v, cand = knn_model(sig, bands, rows, 200, thr)     # 200 > n - 1: every candidate of every row
        degs = np.array([len(r) for r in cand])
        assert degs.max() > 5 and degs.min() == 0 and ((degs > 0) & (degs < 5)).any()
        for top in (1, 5, 149, 200):
            same_lists(device_lists(sig, bands, rows, top, thr, ld=n_hash + 5), [r[:top] for r in full_i], [r[:top] for r in full_v])
            assert similarity.mh_lsh_last_route()["edges"] == int(np.minimum(degs, top).sum())


def test_all_rows_equal(da):
    eq = np.tile(random_sig(1, 1, 48), (130, 1))
    for top in (5, 129, 200):
        idx, val = device_lists(eq, 12, 4, top, ld=64)
        others = np.array([[j for j in range(130) if j != i][:top] for i in range(130)])
        assert np.array_equal(idx[:, :others.shape[1]], others) and (idx[:, others.shape[1]:] == -1).all()
        assert (val[:, :others.shape[1]] == 1.0).all() and (val[:, others.shape[1]:] == 0.0).all()
    # a row longer than top = 1024 and than a wave, shorter than the LDS buffer: row i lists 0 .. 1024 without i (closed form)
    eq = np.tile(random_sig(2, 1, 8), (1100, 1))
    idx, val = device_lists(eq, 2, 4, 1024)
    i = np.arange(1100)[:, None]
    t = np.arange(1024)[None, :]
    assert np.array_equal(idx, np.where(t < i, t, t + 1)) and (val == 1.0).all()


def test_all_rows_distinct(da):
    from dynaalign_amd import similarity
    distinct = random_sig(2, 130, 48)
    assert model(distinct, 12, 4, 0.0)["incidences"] == 0
    idx, val = device_lists(distinct, 12, 4, 7)
    assert idx.shape == (130, 7) and (idx == -1).all() and (val == 0.0).all()
    assert similarity.mh_lsh_last_route()["edges"] == 0
    idx, val = device_lists(distinct[:1], 12, 4, 1024)                   # n = 1: one row of padding, top not clamped
    assert idx.shape == (1, 1024) and (idx == -1).all() and (val == 0.0).all()


def test_cap_and_refusals_on_the_device_entry(da):
    from dynaalign_amd import device
    sig = np.tile(random_sig(4, 1, 31), (20, 1))
    t = to_device(sig, 32)
    with pytest.raises(da.DynaAlignError) as e:
        device.lsh_knn(t, 31, 5, 6, 3, max_candidates=5 * 190 - 1)
    assert e.value.code == UNSUPPORTED and "950" in str(e.value) and "largest bucket: 20" in str(e.value)
    idx, _ = device.lsh_knn(t, 31, 5, 6, 3, max_candidates=5 * 190)
    assert idx.cpu().tolist() == [[j for j in range(20) if j != i][:3] for i in range(20)]
    with pytest.raises(da.DynaAlignError) as e:
        device.lsh_knn(t, 31, 5, 6, 1025)
    assert str(e.value) == "top must be in 1 .. 1024 (got 1025)"


# ---- the host entry ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params,fam", CASES[:3], ids=["12x4", "10x5", "33x3"])
def test_host_entry_equals_the_definition_on_oracle_signatures(da, params, fam):
    from dynaalign_amd import similarity
    k, n_hash, bands, rows, thr = params
    seqs = family(*fam) + FIXED
    sig = oracle_sig(seqs, k, n_hash)
    want = model(sig, bands, rows, 0.0)
    assert want["incidences"] > 0 and want["multi"] > 0
    for top in (3, 10):
        for threshold in (0.0, thr):
            idx, val = da.similarityMH_lsh_knn(seqs, k, n_hash, bands, rows, top, threshold=threshold, seed=SEED)
            want_i, want_v = da.lsh_knn_dense(sig, bands, rows, top, threshold)
            assert idx.dtype == np.int32 and val.dtype == np.float64 and idx.shape == (len(seqs), top)
            assert np.array_equal(idx, want_i) and np.array_equal(val.view(np.uint64), want_v.view(np.uint64))
            assert np.array_equal(val > 0, idx >= 0) and (idx >= 0).any() and (idx == -1).any()
            route = similarity.mh_lsh_last_route()
            assert route["incidences"] == want["incidences"] and route["verified_pairs"] == len(want["pairs"])
            assert route["edges"] == int((idx >= 0).sum())
    # the Python model agrees with the numpy definition on these signatures as well
    m_i, m_v, _ = knn_model(sig, bands, rows, 3, thr)
    same_lists(da.similarityMH_lsh_knn(seqs, k, n_hash, bands, rows, 3, threshold=thr, seed=SEED), m_i, m_v)
    # default threshold: 0.0
    a = da.similarityMH_lsh_knn(seqs, k, n_hash, bands, rows, 3, seed=SEED)
    b = da.similarityMH_lsh_knn(seqs, k, n_hash, bands, rows, 3, threshold=0.0, seed=SEED)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_one_band_per_hash_gives_the_all_pairs_lists(da):
    """rows = 1, bands = n_hash: every pair with a count >= 1 is a candidate, so the lists are similarityMH_knn's -- another code path (the
    all-pairs compare and the dense top-k) -- wherever its value is > 0, and padding where it lists a 0"""
    seqs = family(5, 6, 20, 300) + FIXED
    for top in (10, 1):
        ref_i, ref_v = da.similarityMH_knn(seqs, 4, 40, top, seed=SEED)
        idx, val = da.similarityMH_lsh_knn(seqs, 4, 40, 40, 1, top, seed=SEED)
        live = ref_v > 0
        assert live.any() and ((~live).any() or top == 1)
        assert np.array_equal(idx[live], ref_i[live]) and np.array_equal(val[live].view(np.uint64), ref_v[live].view(np.uint64))
        assert (idx[~live] == -1).all() and (val[~live] == 0.0).all()


def test_more_candidates_than_the_cap_is_refused_with_the_count(da):
    seqs = family(1, 6, 20, 300) + FIXED + ["ACDEFGHIKLMNPQRSTVWA"] * 300
    sig = oracle_sig(seqs, 4, 48)
    incidences, largest = 0, 0
    for t in range(12):                                                   # pairs of members of one bucket, summed over the buckets
        _, sizes = np.unique(sig[:, 4 * t:4 * t + 4], axis=0, return_counts=True)
        incidences += int((sizes * (sizes - 1) // 2).sum())
        largest = max(largest, int(sizes.max()))
    assert largest >= 300 and incidences >= 12 * 44850
    with pytest.raises(da.DynaAlignError) as e:
        da.similarityMH_lsh_knn(seqs, 4, 48, 12, 4, 5, seed=SEED, max_candidates=1000)
    assert e.value.code == UNSUPPORTED
    text = str(e.value)
    assert str(incidences) in text and "max_candidates = 1000" in text and "largest bucket: %d" % largest in text
    idx, val = da.similarityMH_lsh_knn(seqs, 4, 48, 12, 4, 5, seed=SEED, max_candidates=incidences)          # exactly the count is enough
    assert idx[305:].tolist() == [[j for j in range(305, 605) if j != i][:5] for i in range(305, 605)] and (val[305:] == 1.0).all()
    with pytest.raises(da.DynaAlignError):
        da.similarityMH_lsh_knn(seqs, 4, 48, 12, 4, 5, seed=SEED, max_candidates=incidences - 1)


# ---- session and clusterbreak -----------------------------------------------------------------------------------------------------------
def test_session_equals_the_host_call_on_a_subset(da):
    from dynaalign_amd import session
    seqs = family(1, 6, 20, 300) + FIXED
    s = session.MinHashSession(seqs, 4, 48, seed=SEED, reserve=False)
    idx = np.random.RandomState(9).permutation(len(seqs))[:173]
    for sub, ix in ((seqs, None), ([seqs[t] for t in idx], idx)):
        for top, thr in ((10, 0.0), (3, 0.5), (400, 0.0)):
            want = da.similarityMH_lsh_knn(sub, 4, 48, 12, 4, top, threshold=thr, seed=s.seed)
            got = s.lsh_knn(12, 4, top, idx=ix, threshold=thr)
            assert (want[0] >= 0).any() and (want[0] == -1).any()
            assert got[0].dtype == np.int32 and got[1].dtype == np.float64
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))
    with pytest.raises(da.DynaAlignError) as e:
        s.lsh_knn(12, 4, max_candidates=10)
    assert e.value.code == UNSUPPORTED
    # the CSR form is the graph of those lists with the 1.0 diagonal
    from dynaalign_amd.clusterbreak import _csr_to_edges
    for mode in ("union", "mutual"):
        thr, n_edges, ptr, adj, codes, loops, values = s.lsh_knn_csr(12, 4, idx, 5, mode)
        want = da.similarityMH_lsh_knn_edges([seqs[t] for t in idx], 4, 48, 12, 4, 5, mode, seed=s.seed)
        ei, ej, ew = _csr_to_edges(ptr, adj, codes, loops, values)
        assert thr == want[0] and n_edges == len(want[1]) > len(idx)
        assert np.array_equal(ei, want[1]) and np.array_equal(ej, want[2]) and np.array_equal(ew.view(np.uint64), want[3].view(np.uint64))


def test_clusterbreak_on_the_lsh_knn_graph(da):
    from dynaalign_amd import session
    from dynaalign_amd.similarity import _knn_edges_result
    pep = family(1, 6, 20, 300)

    def dense_fn(sub):
        idx, val = da.lsh_knn_dense(oracle_sig(sub, 4, 48), 12, 4, min(5, len(sub) - 1))
        return _knn_edges_result(idx, val, 1.0, "union")
    s = session.MinHashSession(pep, 4, 48, seed=SEED, reserve=False)
    a = da.clusterbreak(pep, size_max=40, session=s, knn=5, knn_lsh=(12, 4))
    b = da.clusterbreak(pep, size_max=40, edges_fn=dense_fn)
    c = da.clusterbreak(pep, size_max=40, edges_fn=lambda sub: da.similarityMH_lsh_knn_edges(sub, 4, 48, 12, 4, 5, seed=SEED))
    for other in (a, c):
        assert np.array_equal(other["clustered_seq"], b["clustered_seq"]) and other["filtered_seq"] == b["filtered_seq"]
        assert other.calls == b.calls >= 1 and [l["edges"] for l in other.levels] == [l["edges"] for l in b.levels]
        assert np.array_equal([l["threshold"] for l in other.levels], [l["threshold"] for l in b.levels], equal_nan=True)
    assert len(b.levels) >= 1 and b.levels[0]["edges"] > len(pep)
