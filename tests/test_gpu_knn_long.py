"""GPU tests of the nearest-neighbour lists and the top-k for sequences of up to 1024 residues: the selection kernel on 32-bit value ranks
(device.topk_ranks, plain and with a row's own column excluded) against numpy on the keys and against the 16-bit selection;
similarityNW_knn_long / similarityNW_cross_topk_long through the Python mirror and the raw C calls against the CPU oracle's dense matrix
(knn_dense, argsort), their row blocks, their agreement with the short calls, and similarityNW_knn_edges_long under clusterbreak.  Every
comparison is exact: indices as integers, values and diagonals as uint64 bit patterns."""
import functools

import numpy as np
import pytest
import torch

import oracle_lib as O
from test_gpu_cross import bits, strided, switches
from test_gpu_nw_edges_long import SCORING, far_input, fit, mutate, rand_seq, rank_layouts, square_input, square_oracle, u32
from test_gpu_topk import nw_sets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    from dynaalign_amd import _capi
    assert _capi.load().da_device_count() > 0
    return dynaalign_amd


# ---- 1. the selection kernel alone ---------------------------------------------------------------------------------------------------------------

ROWS = 9
NBINS = (2, 200, 8193, 65536, 65537, 1301496, 2 ** 31 - 1)      # one to four digits; 65537: the top digit of three has a single bit


def digits_of(nbins):
    return max(1, -(-int(nbins - 1).bit_length() // 8))


def rank_block(rng, n, col0, nbins):
    """ROWS rows of n keys below nbins for a block whose row r owns column col0 + r (col0 None: the plain form).  Rows: one key; all zero;
    the own element the unique maximum; the own element among the ties at the rank of the top-th element (the same key on both sides of
    it, three larger ones above); heavy ties with many zeros; keys that agree in every digit but the lowest; ... but the highest; c and
    c + 65536 mixed (a 16-bit truncation would tie them); increasing"""
    hi = int(nbins)
    own0 = 0 if col0 is None else col0
    keys = rng.randint(0, max(hi - 1, 1), (ROWS, n)).astype(np.uint32)
    keys[0] = 123 % hi
    keys[1] = 0
    if 0 <= own0 + 2 < n:
        keys[2, own0 + 2] = hi - 1                                                   # every other key of the row is < hi - 1
    base, above = min(5, hi - 2), min(9, hi - 1)
    keys[3] = base
    for c in rng.randint(0, n, 3):
        if c != own0 + 3:
            keys[3, c] = above
    keys[4] = rng.randint(0, min(4, hi), n)
    keys[4, rng.rand(n) < 0.5] = 0
    top_part = ((hi - 1) >> 8) << 8
    keys[5] = top_part + rng.randint(0, min(256, hi - top_part), n)
    shift = 8 * (digits_of(hi) - 1)
    keys[6] = (rng.randint(0, max((hi - 1) >> shift, 1), n).astype(np.int64) << shift) | int(rng.randint(0, min(1 << shift, hi)))
    step = 65536 if hi > 65536 else (256 if hi > 256 else 1)
    keys[7] = min(7, hi - 1 - step) + step * rng.randint(0, 2, n)
    keys[8] = (np.arange(n) % hi).astype(np.uint32)
    assert int(keys.max()) < hi
    return keys


def run_ranks(keys, top, nbins, ld, offset, col0):
    from dynaalign_amd import device
    rows, n = keys.shape
    buf, view = strided(rows, n, ld, torch.int32, offset)
    view.copy_(torch.from_numpy(keys.view(np.int32)).cuda())
    what = ("topk_ranks", keys.shape, top, nbins, ld, offset, col0)
    r = keys.astype(np.int64)
    if col0 is None:
        idx, key = device.topk_ranks(view, top, nbins)
    else:
        idx, key, own = device.topk_ranks(view, top, nbins, self_col0=col0, want_self=True)
        cols = col0 + np.arange(rows)
        has = (cols >= 0) & (cols < n)
        r[np.nonzero(has)[0], cols[has]] = -1                          # below every rank: never among the top <= n - 1
    torch.cuda.synchronize()
    idx, key = idx.cpu().numpy(), u32(key)
    want = np.argsort(-r, axis=1, kind="stable")[:, :top]
    bad = np.argwhere(idx != want)
    assert idx.dtype == np.int32 and idx.shape == want.shape, what
    assert len(bad) == 0, what + (bad[0].tolist(), idx[bad[0][0]][:12], want[bad[0][0]][:12], keys[bad[0][0]][want[bad[0][0]][:12]])
    assert np.array_equal(key, np.take_along_axis(keys, want, axis=1)), what
    if col0 is not None:
        own = u32(own)
        assert np.array_equal(own[has], keys[np.nonzero(has)[0], cols[has]]) and not own[~has].any(), what   # the own element; untouched elsewhere
    # the key block is only read: the sentinel fill around and between its rows is intact, and so are the keys
    pad = torch.ones(buf.numel(), dtype=torch.bool, device="cuda")
    torch.as_strided(pad, (rows, n), (ld, 1), offset).fill_(False)
    assert bool((buf[pad] == -7).all()) and np.array_equal(u32(view.contiguous()), keys), what


@pytest.mark.parametrize("n", [2, 3, 7, 64, 1024, 1025, 2048, 4099])
def test_topk_ranks_layouts_digits_and_own_columns(da, n):
    rng = np.random.RandomState(n)
    turn = 0
    # own columns from 0; ending at n - 1; inside a 16-byte unit; row 0 at -1; the last row at n; and the plain form
    for col0 in sorted({0, n - ROWS, 3, -1, n - ROWS + 1}) + [None]:
        blocks = {nbins: rank_block(rng, n, col0, nbins) for nbins in NBINS}
        for top in sorted({1, min(10, n - 1), min(1024, n - 1)}):
            for ld, offset in rank_layouts(n):
                nbins = NBINS[turn % len(NBINS)]                      # 5 layouts x 7 digit placements: every pairing comes up
                turn += 1
                run_ranks(blocks[nbins], top, nbins, ld, offset, col0)
    assert turn >= len(NBINS) * 2
    for nbins in NBINS:                                                # every digit placement on the aligned layout, own columns inside the row
        col0 = max(n - ROWS, 0)
        run_ranks(rank_block(rng, n, col0, nbins), min(10, n - 1), nbins, -(-n // 4) * 4, 0, col0)


def test_topk_ranks_top_equal_n_and_the_self_form_refuses_it(da):
    from dynaalign_amd import device
    keys = torch.from_numpy((np.arange(40, dtype=np.int32).reshape(4, 10) * 70000).copy()).cuda()
    with pytest.raises(da.DynaAlignError) as e:
        device.topk_ranks(keys, 10, 2 ** 22, self_col0=0)
    assert e.value.code == 11 and "n - 1" in str(e.value)
    idx, key = device.topk_ranks(keys, 10, 2 ** 22)                  # top = n through the plain form
    assert np.array_equal(idx.cpu().numpy(), np.tile(np.arange(9, -1, -1, dtype=np.int32), (4, 1)))
    assert np.array_equal(key.cpu().numpy(), keys.cpu().numpy()[:, ::-1])
    idx, key = device.topk_ranks(keys, 9, 2 ** 22, self_col0=100)    # no own column in range: the plain selection
    assert np.array_equal(idx.cpu().numpy(), np.tile(np.arange(9, 0, -1, dtype=np.int32), (4, 1)))


# ---- 2. the 16-bit and the 32-bit selection agree --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1024, 1025])
def test_selection_on_16_and_32_bit_keys_agree(da, n):
    from dynaalign_amd import device
    rng = np.random.RandomState(n + 16)
    keys = rng.randint(0, 65536, (8, n)).astype(np.uint16)
    keys[1] = rng.randint(0, 3, n)
    keys[2, rng.rand(n) < 0.7] = 0
    keys[3] = 65535
    k16 = torch.from_numpy(keys.view(np.int16)).cuda()
    k32 = torch.from_numpy(keys.astype(np.uint32).view(np.int32)).cuda()
    for top in (1, 10, 1024):
        a_idx, a_key = device.topk_rows(k16, top, None, 16)
        b_idx, b_key = device.topk_ranks(k32, top, 65536)
        assert torch.equal(a_idx, b_idx)
        assert np.array_equal(a_key.cpu().numpy().view(np.uint16).astype(np.uint32), u32(b_key))
        for col0 in (0, n - 8, 5):
            t = min(top, n - 1)
            a_idx, a_key, a_own = device.topk_rows(k16, t, None, 16, self_col0=col0, want_self=True)
            b_idx, b_key, b_own = device.topk_ranks(k32, t, 65536, self_col0=col0, want_self=True)
            assert torch.equal(a_idx, b_idx)
            assert np.array_equal(a_key.cpu().numpy().view(np.uint16).astype(np.uint32), u32(b_key))
            assert np.array_equal(a_own.cpu().numpy().view(np.uint16).astype(np.uint32), u32(b_own))


# ---- inputs, the oracle, the raw calls ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tie_family():
    """P against P + Q (128/256) and against P[:64] + R (64/128), P2 against P2[:75] + R2 (75/150) and against P2 + Q2 (150/300): four
    times 0.5 from four codes, listed once in each code order"""
    rng = np.random.RandomState(5150)
    P, Q, R = rand_seq(rng, 128, "ACDEFGH"), rand_seq(rng, 128, "KLMNPQRS"), rand_seq(rng, 64, "KLMNPQRS")
    P2, Q2, R2 = rand_seq(rng, 150, "ACDEFGH"), rand_seq(rng, 150, "KLMNPQRS"), rand_seq(rng, 75, "KLMNPQRS")
    return (P, P + Q, P[:64] + R, P2[:75] + R2, P2 + Q2, P2)


@functools.lru_cache(maxsize=None)
def one_set_input():
    seqs = tuple(square_input()) + tie_family() + ("A", "AC", "W", "WW", "ACD")
    assert len(seqs) == 55 and max(map(len, seqs)) == 300
    return seqs


ROW_P, ROW_P2 = 44, 49                                                 # where P and P2 sit among the 55


def host_knn(seqs, matrix, go, ge, top, with_val=True, with_diag=True, entry="da_similarity_nw_knn_long"):
    from dynaalign_amd import _capi
    res, off = O.pack(list(seqs))
    idx, val, diag = np.full((len(seqs), top), -7, np.int32), np.full((len(seqs), top), -7.0), np.full(len(seqs), -7.0)
    _capi.check(getattr(_capi.load(), entry)(res.ctypes.data, off.ctypes.data, len(seqs), matrix.encode(), go, ge, top, idx.ctypes.data,
                                             val.ctypes.data if with_val else None, diag.ctypes.data if with_diag else None))
    return idx, val, diag


def host_cross(x, y, matrix, go, ge, top, with_val=True, entry="da_similarity_nw_cross_topk_long"):
    from dynaalign_amd import _capi
    xr, xo = O.pack(list(x))
    yr, yo = O.pack(list(y))
    idx, val = np.full((len(x), top), -7, np.int32), np.full((len(x), top), -7.0)
    _capi.check(getattr(_capi.load(), entry)(xr.ctypes.data, xo.ctypes.data, len(x), yr.ctypes.data, yo.ctypes.data, len(y), matrix.encode(), go, ge,
                                             top, idx.ctypes.data, val.ctypes.data if with_val else None))
    return idx, val


def assert_lists(got, S, top, what):
    from dynaalign_amd import knn_dense
    assert_rows(got, knn_dense(S, top), what)


def assert_rows(got, want, what):
    idx, val = got
    want_idx, want_val = want
    idx = np.asarray(idx)
    assert idx.dtype == np.int32 and idx.shape == want_idx.shape, (what, idx.dtype, idx.shape, want_idx.shape)
    bad = np.argwhere(idx != want_idx)
    assert len(bad) == 0, (what, "first index difference at", bad[0].tolist(), idx[bad[0][0]][:12], want_idx[bad[0][0]][:12])
    if val is not None:
        val = np.asarray(val)
        assert val.dtype == np.float64 and np.array_equal(bits(val), bits(want_val)), (what, "values differ")


@functools.lru_cache(maxsize=None)
def rect_oracle(x, y, matrix, go, ge):
    """the oracle's rectangle calc(x[i], y[j]), x[i] as sequence1"""
    m = len(x)
    rc, nm, ln, _, msg = O.nw_rows(list(x) + list(y), 0, m, matrix, go, ge)
    assert rc == 0, msg
    R = nm[:, m:].astype(np.float64) / ln[:, m:].astype(np.float64)
    R.setflags(write=False)
    return R


def rect_expected(R, top):
    idx = np.argsort(-R, axis=1, kind="stable")[:, :top]
    return idx.astype(np.int32), np.take_along_axis(R, idx, axis=1)


def selected_ranks(da, S, nm, ln, top, max_len):
    """the value ranks of the entries knn_dense selects"""
    _, table = da.nw_value_ranks(max_len)
    idx, _ = da.knn_dense(S, top)
    rk = table[ln, nm].astype(np.int64)
    return np.take_along_axis(rk, idx.astype(np.int64), axis=1), rk


# ---- 3. one set against the oracle -----------------------------------------------------------------------------------------------------------------

def test_one_set_input_has_cut_ties_in_both_code_orders_and_ranks_past_16_bits(da):
    seqs = one_set_input()
    fam = tie_family()
    assert seqs[ROW_P] == fam[0] and seqs[ROW_P2] == fam[5]
    S, nm, ln = square_oracle(seqs, "BLOSUM62", 10, 4)
    n = len(seqs)
    assert np.array_equal(bits(S), bits(S.T))
    idx, val = da.knn_dense(S, 2)
    # row P lists P + Q (128/256) then P[:64] + R (64/128); row P2 lists P2[:75] + R2 (75/150) then P2 + Q2 (150/300): at top = 1 the cut
    # falls between equal values of different codes and position decides, with the larger code kept in one row and cut in the other
    assert idx[ROW_P].tolist() == [45, 46] and idx[ROW_P2].tolist() == [47, 48] and (val[[ROW_P, ROW_P2]] == 0.5).all()
    assert [(int(nm[ROW_P, j]), int(ln[ROW_P, j])) for j in (45, 46)] == [(128, 256), (64, 128)]
    assert [(int(nm[ROW_P2, j]), int(ln[ROW_P2, j])) for j in (47, 48)] == [(75, 150), (150, 300)]
    M = S.copy()
    np.fill_diagonal(M, -np.inf)
    order = np.argsort(-M, axis=1, kind="stable")
    code = (nm.astype(np.int64) << 16) | ln
    r = np.arange(n)
    for top, least in ((1, 2), (10, 3)):                               # rows whose cut at `top` separates equal values of different codes
        a, b = order[:, top - 1], order[:, top]
        assert int(((S[r, a] == S[r, b]) & (code[r, a] != code[r, b])).sum()) >= least, top
    sel, rk = selected_ranks(da, S, nm, ln, 10, 300)
    assert int((rk[~np.eye(n, dtype=bool)] >= 65536).sum()) >= 10 and int((sel >= 65536).sum()) >= 10     # a 16-bit rank would not hold them
    S50, nm50, ln50 = square_oracle(seqs, "BLOSUM50", 11, 1)           # there the ties dissolve (64/130): asserted for BLOSUM62 only
    assert (int(nm50[ROW_P, 46]), int(ln50[ROW_P, 46])) == (64, 130)


@pytest.mark.parametrize("matrix,go,ge", SCORING, ids=[s[0] for s in SCORING])
def test_one_set_against_the_oracle(da, matrix, go, ge):
    seqs = one_set_input()
    S, _, _ = square_oracle(seqs, matrix, go, ge)
    diag = np.diag(S).copy()
    for top in (1, 10, 54):
        assert_lists(da.similarityNW_knn_long(list(seqs), matrix, go, ge, top), S, top, ("mirror", matrix, top))
        idx, val, dg = host_knn(seqs, matrix, go, ge, top)
        assert_lists((idx, val), S, top, ("host", matrix, top))
        assert np.array_equal(bits(dg), bits(diag))
    idx, val, dg = host_knn(seqs, matrix, go, ge, 10, with_val=False, with_diag=False)
    assert_lists((idx, None), S, 10, ("host, idx only", matrix))
    assert (val == -7.0).all() and (dg == -7.0).all()
    idx, val, dg = host_knn(seqs, matrix, go, ge, 10, with_diag=False)
    assert_lists((idx, val), S, 10, ("host, no diagonal", matrix))
    assert_lists(da.similarityNW_knn_long(list(seqs), matrix, go, ge, 300), S, 54, ("mirror, clamped", matrix))


# ---- 4. the far end ---------------------------------------------------------------------------------------------------------------------------------

def test_far_end_third_digit_decides(da):
    seqs = far_input()
    assert max(map(len, seqs)) == 1024
    S, nm, ln = square_oracle(seqs, "BLOSUM62", 10, 4)
    values, _ = da.nw_value_ranks(1024)
    sel, rk = selected_ranks(da, S, nm, ln, 5, 1024)
    assert len(values) == 956758 and int(rk.max()) == 956757 and int(sel[:, 0].max()) >= 2 ** 16   # three digits, and the third one decides
    for top in (1, 5):
        assert_lists(da.similarityNW_knn_long(list(seqs), top=top), S, top, ("far, mirror", top))
        idx, val, dg = host_knn(seqs, "BLOSUM62", 10, 4, top)
        assert_lists((idx, val), S, top, ("far, host", top))
        assert np.array_equal(bits(dg), bits(np.diag(S).copy()))
        assert_rows(da.similarityNW_cross_topk_long(list(seqs[:2]), list(seqs), top=top), rect_expected(rect_oracle(seqs[:2], seqs, "BLOSUM62", 10, 4), top),
                    ("far, two sets", top))


# ---- 5. two sets against the oracle -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("matrix,go,ge", SCORING, ids=[s[0] for s in SCORING])
def test_two_sets_against_the_oracle(da, matrix, go, ge):
    seqs = one_set_input()
    x, y = seqs[40:50], seqs
    R = rect_oracle(x, y, matrix, go, ge)                               # x[i] is sequence1: NOT rows of the one-set matrix, which mirrors calc(seq[min], seq[max])
    if matrix == "BLOSUM62":                                           # the cut tie at top = 2: the row's copy at 1.0, then one of two 0.5s
        idx, val = rect_expected(R, 3)
        assert idx[ROW_P - 40].tolist() == [44, 45, 46] and idx[ROW_P2 - 40].tolist() == [49, 47, 48]
        assert val[ROW_P - 40].tolist() == [1.0, 0.5, 0.5] and val[ROW_P2 - 40].tolist() == [1.0, 0.5, 0.5]
    for top in (1, 2, 10, 55):
        want = rect_expected(R, top)
        assert_rows(da.similarityNW_cross_topk_long(list(x), list(y), matrix, go, ge, top), want, ("mirror", matrix, top))
        assert_rows(host_cross(x, y, matrix, go, ge, top), want, ("host", matrix, top))
    idx, val = host_cross(x, y, matrix, go, ge, 10, with_val=False)
    assert_rows((idx, None), rect_expected(R, 10), ("host, idx only", matrix))
    assert (val == -7.0).all()
    assert_rows(da.similarityNW_cross_topk_long(list(x), list(y), matrix, go, ge, 300), rect_expected(R, 55), ("mirror, clamped", matrix))


# ---- 6. row blocks ---------------------------------------------------------------------------------------------------------------------------------------

def test_row_blocks_give_identical_results(da):
    seqs = one_set_input()
    x, y = seqs[40:50], seqs
    S, _, _ = square_oracle(seqs, "BLOSUM62", 10, 4)
    top = 10
    whole = host_knn(seqs, "BLOSUM62", 10, 4, top)                      # the symmetric sweep
    cross_whole = host_cross(x, y, "BLOSUM62", 10, 4, top)
    with switches(DYNAALIGN_BLOCK_BYTES=1800):                          # rows of 56 keys of 4 bytes: 8-row blocks, self_col0 = 0, 8, .. 48
        blocked = host_knn(seqs, "BLOSUM62", 10, 4, top)
        cross_blocked = host_cross(x, y, "BLOSUM62", 10, 4, top)        # 2 blocks
        mirror = da.similarityNW_knn_long(list(seqs), top=top)
    assert_lists(blocked[:2], S, top, "blocked")
    assert_lists(mirror, S, top, "blocked, mirror")
    assert np.array_equal(bits(blocked[2]), bits(np.diag(S).copy()))
    assert np.array_equal(whole[0], blocked[0]) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(whole[1:], blocked[1:]))
    assert_rows(cross_blocked, rect_expected(rect_oracle(x, y, "BLOSUM62", 10, 4), top), "two sets, blocked")
    assert np.array_equal(cross_whole[0], cross_blocked[0]) and np.array_equal(bits(cross_whole[1]), bits(cross_blocked[1]))


# ---- 7. continuity with the short calls -------------------------------------------------------------------------------------------------------------

def test_long_calls_equal_the_short_calls_up_to_127_residues(da):
    x, y = nw_sets(np.random.RandomState(31), 40, 90)
    seqs = x + y
    assert max(map(len, seqs)) <= 127
    rc, S, msg = O.similarity_nw(seqs, "BLOSUM62", 10, 4)
    assert rc == 0, msg
    first = np.argsort(-S, axis=1, kind="stable")[:, 0]
    assert int((first != np.arange(len(seqs))).sum()) >= 1            # rows whose own column is not the first of its ties
    for top in (1, 10, len(seqs) - 1):
        a, b = da.similarityNW_knn(seqs, top=top), da.similarityNW_knn_long(seqs, top=top)
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
        ha, hb = host_knn(seqs, "BLOSUM62", 10, 4, top, entry="da_similarity_nw_knn"), host_knn(seqs, "BLOSUM62", 10, 4, top)
        assert np.array_equal(ha[0], hb[0]) and np.array_equal(bits(ha[1]), bits(hb[1])) and np.array_equal(bits(ha[2]), bits(hb[2]))
    for top in (1, 10, len(y) - 1):
        a, b = da.similarityNW_cross_topk(x, y, top=top), da.similarityNW_cross_topk_long(x, y, top=top)
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


# ---- 8. graph and clustering ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["union", "mutual"])
def test_knn_edges_long_equal_knn_graph(da, mode):
    seqs = one_set_input()
    S, _, _ = square_oracle(seqs, "BLOSUM62", 10, 4)
    thr, i, j, w = da.similarityNW_knn_edges_long(list(seqs), top=10, mode=mode)
    wi, wj, ww = da.knn_graph(*da.knn_dense(S, 10), np.diag(S).copy(), mode)
    assert np.array_equal(i, wi) and np.array_equal(j, wj) and np.array_equal(bits(w), bits(ww))
    assert len(ww[wi != wj]) > 0 and thr == ww[wi != wj].min()         # the threshold slot: the smallest off-diagonal weight


def test_clusterbreak_on_the_long_knn_graph_and_consensus(da):
    rng = np.random.RandomState(2024)
    parents = [rand_seq(rng, 200) for _ in range(3)]
    pep = [fit(rng, mutate(rng, parents[t % 3], 0.04 + 0.02 * (t % 5)), int(rng.randint(130, 201))) for t in range(60)]
    assert min(map(len, pep)) >= 130 and max(map(len, pep)) <= 200

    def dense_edges(s):
        S = np.asarray(da.similarityNW(s))
        ei, ej, w = da.knn_graph(*da.knn_dense(S, min(8, len(s) - 1)), np.diag(S).copy(), "union")
        return float(w[ei != ej].min()), ei, ej, w
    a = da.clusterbreak(pep, size_max=25, edges_fn=lambda s: da.similarityNW_knn_edges_long(s, top=8), cluster_seed=2)
    b = da.clusterbreak(pep, size_max=25, edges_fn=dense_edges, cluster_seed=2)
    assert np.array_equal(a["clustered_seq"], b["clustered_seq"]) and a["filtered_seq"] == b["filtered_seq"]
    assert a.calls == b.calls and len(a.levels) == len(b.levels) >= 1 and [l["edges"] for l in a.levels] == [l["edges"] for l in b.levels]
    assert all(l["edges"] <= l["n"] * 9 for l in a.levels)              # at most n * top edges + the diagonal
    rows = a["clustered_seq"]
    assert len(rows) > 0
    cons = da.clusterconsensus(rows, align_fn=da.nw_align_long)
    ids = list(dict.fromkeys(r[1] for r in rows))
    assert [c[0] for c in cons] == ids and all(isinstance(c[1], str) for c in cons)
