"""GPU tests of the NW-ranked nearest-neighbour lists on MinHash LSH candidates: the selection on 32-bit keys (lsh_kernels.hip:
k_lsh_knn_select_short / _long <uint32_t>), the rank-key step (nw_lsh_kernels.hip: k_nwl_rank_keys), the host entries similarityNW_lsh_knn /
similarityNW_lsh_knn_edges / similarityNW_lsh_cross_topk, the device routes and clusterbreak on the graph.  Every comparison is exact --
indices as integers, values as uint64 bit patterns.  The expected values come from numpy sorts of the rows and from the oracle's pair
value on the candidates of the LSH models of test_lsh_cpu.py / test_lsh_cross_cpu.py over the oracle's signatures, never from the code
under test."""
import numpy as np
import pytest
import torch

import oracle_lib as O
from test_gpu_jaccard import family
from test_gpu_nw_lsh import BANDINGS, N_HASH, SEED, UNSUPPORTED, PairValues, mixed_set, oracle_sig, rand_seq, short_set
from test_lsh_cpu import model
from test_lsh_cross_cpu import cross_model
from test_nw_lsh_knn_cpu import rows_model, same_lists

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    from dynaalign_amd import _capi
    assert _capi.load().da_device_count() > 0
    return dynaalign_amd


# ---- the selection on synthetic ragged rows ---------------------------------------------------------------------------------------------
EXTREMES = np.array([0, 0xFFFFFFFF, 0x01000000, 0x00FFFFFF, 65536, 65535, 256, 255], np.int64)
PATTERNS = ("equal", "straddle", "extremes", "random", "low_byte")


def degrees_for(top):
    """0, 1, around top, around a wave, one below / at / above the LDS buffer, and two rows for the radix select"""
    from dynaalign_amd import device
    assert (device.LSH_KNN_WAVE_MAX, device.LSH_KNN_LDS_WORDS) == (64, 2048)
    return [0, 1, max(top - 1, 0), top, top + 1, 63, 64, 65, 2047, 2048, 2049, 5000, 70000]


def ragged_rows(degrees, pattern, top, seed):
    """-> (ptr int64, col int32, key uint32): distinct columns from the whole non-negative int32 range in random order, 2^31 - 1 and 0
    among them; keys by pattern"""
    rng = np.random.RandomState(seed)
    ptr = np.zeros(len(degrees) + 1, np.int64)
    ptr[1:] = np.cumsum(degrees)
    cols, keys = [], []
    for deg in degrees:
        c = rng.permutation(np.unique(rng.randint(1, (1 << 31) - 1, deg + 64, dtype=np.int64)))[:deg]
        if deg >= 2:
            c[:2] = 0, (1 << 31) - 1
            c = rng.permutation(c)
        assert len(set(c.tolist())) == deg
        if pattern == "equal":                                         # the column digits alone decide
            v = np.full(deg, 0x12345678, np.int64)
        elif pattern == "straddle":                                    # top - 1 (or half the row) at the high value: position top falls among the low ones
            v = np.full(deg, 0x80000000 - 1, np.int64)
            v[rng.permutation(deg)[:(top - 1 if deg > top else deg // 2)]] = 0x80000000
        elif pattern == "extremes":
            v = rng.choice(EXTREMES, deg)
        elif pattern == "random":
            v = rng.randint(0, 1 << 32, deg, dtype=np.int64)
        else:                                                          # low_byte: one value in the seven digits above, so the radix select walks all eight
            v = 0xA5C3F100 + rng.randint(0, 256, deg, dtype=np.int64)
        cols.append(c)
        keys.append(v)
    return ptr, np.concatenate(cols).astype(np.int32), np.concatenate(keys).astype(np.uint32)


def select_reference(ptr, col, key, top, nnz=None):
    """per row: a numpy sort by (key descending, column ascending) of the entries inside [0, nnz), the first top, then -1 / 0"""
    nnz = len(col) if nnz is None else nnz
    n = len(ptr) - 1
    idx = np.full((n, top), -1, np.int32)
    out = np.zeros((n, top), np.uint32)
    for r in range(n):
        b, e = min(max(int(ptr[r]), 0), nnz), min(max(int(ptr[r + 1]), 0), nnz)
        e = max(e, b)
        c, v = col[b:e].astype(np.int64), key[b:e].astype(np.int64)
        order = np.lexsort((c, -v))[:top]
        idx[r, :len(order)] = c[order]
        out[r, :len(order)] = v[order]
    return idx, out


def run_select(ptr, col, key, top, nnz=None, pad=3):
    from dynaalign_amd import device
    n = len(ptr) - 1
    out_i = torch.full((n, top + pad), 77, dtype=torch.int32, device="cuda")
    out_k = torch.full((n, top + pad), 77, dtype=torch.int32, device="cuda")
    t_ptr, t_col = torch.from_numpy(ptr).cuda(), torch.from_numpy(col).cuda()
    t_key = torch.from_numpy(key.view(np.int32)).cuda()
    idx, got = device.nw_knn_select(t_ptr, t_col, t_key, top, nnz=nnz, out=(out_i, out_k))
    torch.cuda.synchronize()
    assert idx.shape == (n, top) and got.shape == (n, top)
    assert (out_i[:, top:] == 77).all() and (out_k[:, top:] == 77).all()          # the padding columns of the outputs are untouched
    return idx.cpu().numpy(), got.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("top", [1, 10, 64, 1000, 1024])
def test_select_on_synthetic_ragged_rows(da, top):
    for p, pattern in enumerate(PATTERNS):
        ptr, col, key = ragged_rows(degrees_for(top), pattern, top, 100 * top + p)
        assert col.max() == (1 << 31) - 1 and col.min() == 0
        if pattern in ("extremes", "random"):
            assert key.max() >= 0xFF000000 and key.min() < 0x01000000   # the whole uint32 range
        want_i, want_k = select_reference(ptr, col, key, top)
        got_i, got_k = run_select(ptr, col, key, top)
        assert np.array_equal(got_i, want_i), pattern
        assert np.array_equal(got_k, want_k), pattern
        assert np.array_equal(got_i >= 0, np.arange(top)[None, :] < np.minimum(np.diff(ptr), top)[:, None])


def test_select_cuts_rows_to_the_entries_inside_nnz_and_refuses(da):
    """a clamp on valid memory: col / key are allocated at full length, a smaller nnz is passed, and one row's pointer runs backwards"""
    from dynaalign_amd import device
    degrees = [3, 70, 10, 3000, 40, 5, 100]
    ptr, col, key = ragged_rows(degrees, "random", 10, 6)
    nnz = int(ptr[3]) + 1500                                              # inside row 3: rows 4 .. 6 lie behind it
    for top in (10, 1024):
        want_i, want_k = select_reference(ptr, col, key, top, nnz)
        assert (want_i[3] >= 0).sum() == min(1500, top) and (want_i[4:] == -1).all()
        got_i, got_k = run_select(ptr, col, key, top, nnz=nnz)
        assert np.array_equal(got_i, want_i) and np.array_equal(got_k, want_k)
    back = ptr.copy()
    back[2] = ptr[1] - 2                                                  # row 1 runs backwards (empty), row 2 then starts inside row 0
    want_i, want_k = select_reference(back, col, key, 10)
    assert (want_i[1] == -1).all() and (want_i[2] >= 0).all()
    got_i, got_k = run_select(back, col, key, 10)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_k, want_k)
    t = [torch.from_numpy(a).cuda() for a in (ptr, col, key.view(np.int32))]
    idx, got = device.nw_knn_select(*t, 4)                                # outputs allocated by the call, ld = top
    torch.cuda.synchronize()
    want_i, want_k = select_reference(ptr, col, key, 4)
    assert np.array_equal(idx.cpu().numpy(), want_i) and np.array_equal(got.cpu().numpy().view(np.uint32), want_k)
    for bad_top in (0, 1025):
        with pytest.raises(da.DynaAlignError) as e:
            device.nw_knn_select(*t, bad_top)
        assert str(e.value) == "top must be in 1 .. 1024 (got %d)" % bad_top


# ---- the rank-key step on a hand-made list -------------------------------------------------------------------------------------------------
def test_rank_keys_on_a_hand_made_list(da):
    from dynaalign_amd import device
    max_len = 20
    values, rank = da.nw_value_ranks(max_len)
    # (i, j, matches, length): 5/10 and 10/20 (one rank), 0/len (dropped), a diagonal entry, -1/-1, a value under the threshold, 1.0, a code
    # outside the table (length 41 > 2 * max_len), and a pair with i == j where the sets differ (kept when one_set is false)
    listed = [(0, 1, 5, 10), (0, 2, 10, 20), (1, 2, 0, 13), (3, 3, 7, 9), (2, 4, -1, -1), (1, 4, 3, 10), (0, 4, 20, 20), (3, 4, 5, 41), (2, 2, 19, 20),
              (4, 4, 0, 5)]
    cols = [torch.tensor([p[f] for p in listed], dtype=torch.int32, device="cuda") for f in range(4)]
    drank = torch.from_numpy(rank.view(np.int32).copy()).cuda()
    half = int(np.searchsorted(values, 0.5))
    assert values[half] == 0.5 and rank[10, 5] == rank[20, 10] == half and values[0] == 0.0 and rank[13, 0] == 0
    want_key = [half, half, 0, int(rank[9, 7]), 0, int(rank[10, 3]), int(rank[20, 20]), 0, int(rank[20, 19]), 0]
    for r_min, one_set in ((1, True), (half, True), (half + 1, True), (1, False)):
        key, keep, diag, totals = device.nw_rank_keys(*cols, drank, max_len, r_min, one_set, 5)
        torch.cuda.synchronize()
        assert key.cpu().numpy().view(np.uint32).tolist() == want_key
        want_keep = [int(k >= r_min and k > 0 and not (one_set and p[0] == p[1])) for k, p in zip(want_key, listed)]
        assert keep.cpu().tolist() == want_keep
        assert totals.cpu().tolist() == [sum(want_keep), 2]                       # the -1 / -1 pair and the code outside the table
        assert diag.cpu().numpy().view(np.uint32).tolist() == ([0, 0, int(rank[20, 19]), int(rank[9, 7]), 0] if one_set else [0] * 5)
    key, keep, diag, totals = device.nw_rank_keys(*[c[:0] for c in cols], drank, max_len, 1, True, 5)
    assert key.numel() == 0 and totals.cpu().tolist() == [0, 0]


# ---- the host entry against the model ---------------------------------------------------------------------------------------------------------
def knn_set():
    """short_set() and planted ties: q = a + a for a 5-mer a, q + q (q against it: 10 / 20) and q[:5] (5 / 10) -- q + q has q's shingles, q[:5]
    two of its five, so both are candidates of q under either banding for some of the planted q"""
    rng = np.random.RandomState(7)
    seqs = short_set()
    for _ in range(12):
        a = rand_seq(rng, 5)
        seqs += [a + a, a + a + a + a, a]
    seqs = list(dict.fromkeys(seqs))
    return seqs


@pytest.fixture(scope="module")
def knn_case():
    seqs = knn_set()
    return seqs, oracle_sig(seqs), PairValues(seqs, seqs), {}


def cached_model(case, bands, rows, mh_thr):
    seqs, sig, value, cache = case
    if (bands, rows, mh_thr) not in cache:
        cache[(bands, rows, mh_thr)] = model(sig, bands, rows, mh_thr)
    return cache[(bands, rows, mh_thr)]


@pytest.mark.parametrize("mh_thr", [0.0, 0.5])
@pytest.mark.parametrize("bands,rows", BANDINGS, ids=["12x4", "40x1"])
def test_host_entry_equals_the_model(da, knn_case, bands, rows, mh_thr):
    seqs, sig, value, _ = knn_case
    n = len(seqs)
    assert 200 <= n <= 400
    cand = cached_model(knn_case, bands, rows, mh_thr)
    verified = len(cached_model(knn_case, bands, rows, 0.0)["pairs"])
    for thr in (0.0, 0.5):
        full_i, full_v, diag, degs, scored = rows_model(n, cand["i"], cand["j"], value, 1024, thr, True)
        if mh_thr == 0.0:
            # what the inputs were planted for: a row with two candidates of one value and different (matches, length) ...
            ties = 0
            for r in range(n):
                live = [(v, value.ml(min(r, c), max(r, c))) for c, v in zip(full_i[r], full_v[r]) if c >= 0]
                ties += sum(1 for a, b in zip(live, live[1:]) if a[0] == b[0] and a[1] != b[1])
            assert ties > 0
        assert max(degs) > 3                                                  # ... and a row with more than top = 1, 3 candidates
        if rows > 1 or mh_thr > 0:
            assert min(degs) == 0                                             # a row of padding alone
        for top in (1, 3, 1024):
            idx, val = da.similarityNW_lsh_knn(seqs, 4, N_HASH, bands, rows, top, mh_threshold=mh_thr, threshold=thr, seed=SEED)
            assert idx.shape == (n, top) and val.shape == (n, top)
            same_lists((idx, val), [r[:top] for r in full_i], [r[:top] for r in full_v])
            assert np.array_equal(val > 0, idx >= 0)
            route = da.nw_lsh_last_route()
            assert route["aligned_pairs"] == len(cand["i"]) == route["short_pairs"] and route["long_pairs"] == 0
            assert route["edges"] == int(np.minimum(degs, top).sum()) == int((idx >= 0).sum()) and route["verified_pairs"] == verified
            assert route["incidences"] == cached_model(knn_case, bands, rows, 0.0)["incidences"]
        # the edge form carries the scored diagonal
        _, ei, ej, ew = da.similarityNW_lsh_knn_edges(seqs, 4, N_HASH, bands, rows, 3, mh_threshold=mh_thr, threshold=thr, seed=SEED)
        on = ei == ej
        assert on.sum() == n and np.array_equal(ew[on].view(np.uint64), np.array(diag, np.float64).view(np.uint64))


def test_edge_form_equals_knn_graph_of_the_dense_definition(da, knn_case):
    from dynaalign_amd.similarity import _knn_edges_result
    seqs, sig, value, _ = knn_case
    for mode in ("union", "mutual"):
        idx, val, diag = da.nw_lsh_knn_dense(sig, 12, 4, 2, 0.0, value, 0.3)
        want = _knn_edges_result(idx, val, diag, mode)
        got = da.similarityNW_lsh_knn_edges(seqs, 4, N_HASH, 12, 4, 2, mode, threshold=0.3, seed=SEED)
        assert got[0] == want[0] and len(got[1]) > len(seqs)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and np.array_equal(got[3].view(np.uint64), want[3].view(np.uint64))
    union = da.similarityNW_lsh_knn_edges(seqs, 4, N_HASH, 12, 4, 2, threshold=0.3, seed=SEED)
    assert len(union[1]) > len(got[1])                                        # some pair is listed from one side only


def test_the_diagonal_is_scored_and_zero_is_no_entry(da):
    seqs = ["X" * 10, "X" * 20, "ACDEFGHIKLMNPQRSTVWY", "ACDEFGHIKLMNPQRSTVWA", "X" * 9 + "A"]
    value = PairValues(seqs, seqs, 0, 0)
    sig = oracle_sig(seqs)
    want = da.nw_lsh_knn_dense(sig, 12, 4, 4, 0.0, value)
    cand = model(sig, 12, 4, 0.0)
    zero = [(i, j) for i, j in zip(cand["i"], cand["j"]) if i != j and value(i, j) == 0.0]
    assert value(0, 0) < 0.5 and value(2, 2) == 1.0 and len(zero) > 0           # candidates of value 0: scored, never listed
    idx, val = da.similarityNW_lsh_knn(seqs, 4, N_HASH, 12, 4, 4, gapOpen=0, gapExt=0, seed=SEED)
    assert np.array_equal(idx, want[0]) and np.array_equal(val.view(np.uint64), want[1].view(np.uint64))
    assert all(b not in idx[a] and a not in idx[b] for a, b in zero)
    _, ei, ej, ew = da.similarityNW_lsh_knn_edges(seqs, 4, N_HASH, 12, 4, 4, gapOpen=0, gapExt=0, seed=SEED)
    assert np.array_equal(ew[ei == ej].view(np.uint64), want[2].view(np.uint64)) and ew[ei == ej][0] == value(0, 0)


# ---- mixed lengths in one call ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed_case():
    seqs = mixed_set()
    sig = oracle_sig(seqs)
    value = PairValues(seqs, seqs)
    cand = model(sig, 40, 1, 0.0)
    return seqs, sig, value, cand, rows_model(len(seqs), cand["i"], cand["j"], value, 5, 0.0, True)


def test_mixed_lengths_in_one_call_and_in_several_blocks(da, mixed_case, monkeypatch):
    seqs, sig, value, cand, (idx, val, diag, degs, _) = mixed_case
    lens = np.array([len(s) for s in seqs])
    n_long = sum(1 for i, j in zip(cand["i"], cand["j"]) if max(lens[i], lens[j]) > 127)
    got = da.similarityNW_lsh_knn(seqs, 4, N_HASH, 40, 1, 5, seed=SEED)
    same_lists(got, idx, val)
    route = da.nw_lsh_last_route()
    assert route["short_pairs"] == len(cand["i"]) - n_long > 0 and route["long_pairs"] == n_long > 0
    assert route["edges"] == int(np.minimum(degs, 5).sum())
    kinds = {int(lens[r] > 127) + int(lens[c] > 127) for r in range(len(seqs)) for c in idx[r] if c >= 0}
    assert kinds == {0, 1, 2}                                # short-short, short-long and long-long entries in the lists
    monkeypatch.setenv("DYNAALIGN_BLOCK_BYTES", str(1 << 20))
    again = da.similarityNW_lsh_knn(seqs, 4, N_HASH, 40, 1, 5, seed=SEED)
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1].view(np.uint64), got[1].view(np.uint64))


# ---- two sets --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cross_case():
    seqs = mixed_set()
    rng = np.random.RandomState(3)
    order = rng.permutation(len(seqs))
    x = [seqs[t] for t in order[:60]] + [s for s in seqs if len(s) > 127][:6]
    y = [seqs[t] for t in order[40:]]
    return x, y, oracle_sig(x), oracle_sig(y)


def test_two_sets_both_ways_and_sequence1_is_x(da, cross_case):
    x, y, sx, sy = cross_case
    xy, yx = PairValues(x, y), PairValues(y, x)
    cand = cross_model(sx, sy, 40, 1, 0.0)
    cand_t = cross_model(sy, sx, 40, 1, 0.0)
    for top in (2, 1024):
        idx, val, _, degs, scored = rows_model(len(x), cand["i"], cand["j"], xy, top, 0.121, False)
        got = da.similarityNW_lsh_cross_topk(x, y, 4, N_HASH, 40, 1, top, threshold=0.121, seed=SEED)
        same_lists(got, idx, val)
        route = da.nw_lsh_last_route()
        assert route["short_pairs"] > 0 and route["long_pairs"] > 0 and route["aligned_pairs"] == len(cand["i"])
        assert route["edges"] == int(np.minimum(degs, top).sum())
        t_idx, t_val, _, _, t_scored = rows_model(len(y), cand_t["i"], cand_t["j"], yx, top, 0.121, False)
        got_t = da.similarityNW_lsh_cross_topk(y, x, 4, N_HASH, 40, 1, top, threshold=0.121, seed=SEED)
        same_lists(got_t, t_idx, t_val)
    assert max(degs) > 2 and min(degs) == 0
    # the values of the two directions differ exactly where the oracle's depend on the order
    forward = {(i, int(j)): v for i in range(len(x)) for j, v in zip(got[0][i], got[1][i]) if j >= 0}
    backward = {(int(i), j): v for j in range(len(y)) for i, v in zip(got_t[0][j], got_t[1][j]) if i >= 0}
    asymmetric = [p for p in scored if xy.ml(*p) != yx.ml(p[1], p[0])]
    assert len(asymmetric) > 0
    for p in scored:
        want_f, want_b = (xy(*p) if xy(*p) >= 0.121 else None), (yx(p[1], p[0]) if yx(p[1], p[0]) >= 0.121 else None)
        assert forward.get(p) == want_f and backward.get(p) == want_b
        assert (forward.get(p) != backward.get(p)) == (want_f != want_b)
    assert any(forward.get(p) != backward.get(p) for p in asymmetric)


# ---- the device routes on resident data ------------------------------------------------------------------------------------------------------
def test_device_route_equals_the_host_entry_and_the_cap(da, mixed_case):
    from dynaalign_amd import device
    seqs, sig, value, cand, _ = mixed_case
    ds = device.DeviceSequences(*O.pack(seqs))
    device.nw_encode(ds)
    dsig = torch.from_numpy(sig.view(np.int32).copy()).cuda()
    max_len = max(len(s) for s in seqs)
    values, rank = da.nw_value_ranks(max_len)
    drank = torch.from_numpy(rank.view(np.int32).copy()).cuda()
    for top, thr, mh_thr in ((5, 0.2, 0.0), (1024, 0.0, 0.5)):
        want_i = da.similarityNW_lsh_knn(seqs, 4, N_HASH, 40, 1, top, mh_threshold=mh_thr, threshold=thr, seed=SEED)
        host_edges = da.nw_lsh_last_route()["edges"]
        idx, key, diag = device.lsh_nw_knn(dsig, ds, N_HASH, 40, 1, top, drank, max_len, threshold=thr, mh_threshold=mh_thr)
        torch.cuda.synchronize()
        assert device.nw_lsh_last_route()["edges"] == host_edges
        k = key.cpu().numpy().view(np.uint32)
        assert np.array_equal(idx.cpu().numpy(), want_i[0]) and np.array_equal(values[k].view(np.uint64), want_i[1].view(np.uint64))
        assert np.array_equal(k > 0, want_i[0] >= 0)
        d = values[diag.cpu().numpy().view(np.uint32)]
        assert d.tolist() == [value(i, i) for i in range(len(seqs))]
    # the cap on the (pair, band) incidences, with the text of the MinHash call
    incidences = model(sig, 40, 1, 0.0)["incidences"]
    for call in (lambda cap: device.lsh_nw_knn(dsig, ds, N_HASH, 40, 1, 5, drank, max_len, max_candidates=cap),
                 lambda cap: da.similarityNW_lsh_knn(seqs, 4, N_HASH, 40, 1, 5, seed=SEED, max_candidates=cap)):
        with pytest.raises(da.DynaAlignError) as e:
            call(incidences - 1)
        with pytest.raises(da.DynaAlignError) as mh:
            da.similarityMH_lsh_knn(seqs, 4, N_HASH, 40, 1, 5, seed=SEED, max_candidates=incidences - 1)
        assert e.value.code == UNSUPPORTED and str(e.value) == str(mh.value) and "max_candidates = %d" % (incidences - 1) in str(e.value)
        call(incidences)
    # a table shorter than the sequences: the candidates outside it are counted and the call refused
    small_values, small_rank = da.nw_value_ranks(100)
    with pytest.raises(da.DynaAlignError) as e:
        device.lsh_nw_knn(dsig, ds, N_HASH, 40, 1, 5, torch.from_numpy(small_rank.view(np.int32).copy()).cuda(), 100)
    assert e.value.code == UNSUPPORTED and "max_len = 100" in str(e.value)


def test_device_route_for_two_sets(da, cross_case):
    from dynaalign_amd import device
    x, y, sx, sy = cross_case
    dx, dy = device.DeviceSequences(*O.pack(x)), device.DeviceSequences(*O.pack(y))
    device.nw_encode(dx)
    device.nw_encode(dy)
    tx, ty = (torch.from_numpy(s.view(np.int32).copy()).cuda() for s in (sx, sy))
    index = device.lsh_index_build(ty, N_HASH, 40, 1)
    max_len = max(len(s) for s in x + y)
    values, rank = da.nw_value_ranks(max_len)
    drank = torch.from_numpy(rank.view(np.int32).copy()).cuda()
    want = da.similarityNW_lsh_cross_topk(x, y, 4, N_HASH, 40, 1, 3, threshold=0.3, seed=SEED)
    idx, key = device.lsh_nw_cross_topk(index, tx, dx, ty, dy, N_HASH, 40, 1, 3, drank, max_len, threshold=0.3)
    torch.cuda.synchronize()
    assert (want[0] >= 0).any() and (want[0] == -1).any()
    assert np.array_equal(idx.cpu().numpy(), want[0])
    assert np.array_equal(values[key.cpu().numpy().view(np.uint32)].view(np.uint64), want[1].view(np.uint64))


# ---- clusterbreak ------------------------------------------------------------------------------------------------------------------------------
def test_clusterbreak_on_the_nw_lsh_knn_graph(da):
    from dynaalign_amd.similarity import _knn_edges_result
    pep = family(1, 6, 20, 300)

    def dense_fn(sub):
        idx, val, diag = da.nw_lsh_knn_dense(oracle_sig(sub), 12, 4, 5, 0.0, PairValues(sub, sub))
        return _knn_edges_result(idx, val, diag, "union")
    a = da.clusterbreak(pep, size_max=40, edges_fn=lambda s: da.similarityNW_lsh_knn_edges(s, 4, N_HASH, 12, 4, 5, seed=SEED))
    b = da.clusterbreak(pep, size_max=40, edges_fn=dense_fn)
    assert np.array_equal(a["clustered_seq"], b["clustered_seq"]) and a["filtered_seq"] == b["filtered_seq"]
    assert a.calls == b.calls >= 1 and [l["edges"] for l in a.levels] == [l["edges"] for l in b.levels]
    assert np.array_equal([l["threshold"] for l in a.levels], [l["threshold"] for l in b.levels], equal_nan=True)
    assert b.levels[0]["edges"] > len(pep)
