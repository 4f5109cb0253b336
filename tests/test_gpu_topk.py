"""GPU tests of the two-set top-k calls: similarityMH_cross_topk / similarityNW_cross_topk on the host boundary, the one-call device route,
MinHashSession.cross_topk and da_dev_topk_rows on key blocks built here.  Every expected value comes from the oracle on the concatenation
c(x, y) -- the block [0:m, m:m+n], then a stable argsort of its negation -- or, for the selection kernel alone, from numpy on the keys.
All comparisons are exact: indices as integers, values as uint64 bit patterns."""
import numpy as np
import pytest
import torch

import oracle_lib as O
from test_gpu_cross import AA24, SEED, bits, strided, switches, two_sets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    from dynaalign_amd import _capi
    assert _capi.load().da_device_count() > 0
    return dynaalign_amd


def expected(R, top):
    idx = np.argsort(-R, axis=1, kind="stable")[:, :top]
    return idx.astype(np.int32), np.take_along_axis(R, idx, axis=1)


def assert_topk(got, R, top, what):
    idx, val = got
    want_idx, want_val = expected(R, top)
    idx = np.asarray(idx)
    assert idx.dtype == np.int32 and idx.shape == want_idx.shape, (what, idx.dtype, idx.shape)
    bad = np.argwhere(idx != want_idx)
    assert len(bad) == 0, (what, "first index difference at", bad[0].tolist(), idx[bad[0][0]][:12], want_idx[bad[0][0]][:12])
    if val is not None:
        val = np.asarray(val)
        assert val.dtype == np.float64 and np.array_equal(bits(val), bits(want_val)), (what, "values differ")


def host_mh(x, y, k, n_hash, seeds, top, with_val=True):
    from dynaalign_amd import _capi
    xr, xo = O.pack(x)
    yr, yo = O.pack(y)
    idx, val = np.full((len(x), top), -7, np.int32), np.full((len(x), top), -7.0)
    _capi.check(_capi.load().da_similarity_mh_cross_topk(xr.ctypes.data, xo.ctypes.data, len(x), yr.ctypes.data, yo.ctypes.data, len(y), k,
                                                         n_hash, np.ascontiguousarray(seeds, np.uint32).ctypes.data, top, idx.ctypes.data,
                                                         val.ctypes.data if with_val else None))
    return idx, (val if with_val else None)


def host_nw(x, y, matrix, go, ge, top):
    from dynaalign_amd import _capi
    xr, xo = O.pack(x)
    yr, yo = O.pack(y)
    idx, val = np.full((len(x), top), -7, np.int32), np.full((len(x), top), -7.0)
    _capi.check(_capi.load().da_similarity_nw_cross_topk(xr.ctypes.data, xo.ctypes.data, len(x), yr.ctypes.data, yo.ctypes.data, len(y),
                                                         matrix.encode(), go, ge, top, idx.ctypes.data, val.ctypes.data))
    return idx, val


def device_mh(x, y, k, n_hash, seeds, top):
    from dynaalign_amd import device
    dx, dy = device.DeviceSequences(*O.pack(x)), device.DeviceSequences(*O.pack(y))
    idx, val = device.similarity_mh_cross_topk(dx, dy, k, n_hash, seeds, top)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), val.cpu().numpy()


def mh_matrix(x, y, k, n_hash, seeds):
    """R of similarityMH_cross from the oracle: the counts of rows [0, m) of c(x, y), columns [m, m + n), and the reference's divide"""
    m = len(x)
    cnt = O.mh_counts(O.signatures(x + y, k, n_hash, seeds), 0, m)[:, m:]
    return cnt.astype(np.float64) / np.float64(n_hash)


# (m, n, k, n_hash, tops): n_hash = 3000 has ranks above 11 bits, 33 is below 8; (300, 1001) is an odd n; (130, 130900) is the shape where
# m rounded up to 128 would push the joint operand over 131 068 rows, so x stays unpadded
MH_CASES = [(1, 1, 4, 50, (1,)), (3, 5, 1, 33, (1, 2, 5)), (127, 129, 4, 500, (1, 2, 10, 129)), (128, 128, 1, 3000, (1, 10, 128)),
            (300, 1000, 4, 3000, (1, 2, 10, 1000)), (300, 1001, 4, 33, (10, 1001)), (40, 1500, 1, 50, (10, 1024)),
            (2000, 5000, 4, 500, (10, 1024)), (130, 130900, 4, 33, (10,))]


@pytest.mark.parametrize("m,n,k,n_hash,tops", MH_CASES, ids=["%dx%d" % c[:2] for c in MH_CASES])
def test_minhash_every_entry_point_against_the_oracle(da, m, n, k, n_hash, tops):
    from dynaalign_amd import session
    rng = np.random.RandomState(1000 + MH_CASES.index((m, n, k, n_hash, tops)))
    x, y = two_sets(rng, m, n, "ACDEFGHIKLMNPQRSTVWY", high_bytes=True)
    seeds = O.seeds(SEED, n_hash)
    R = mh_matrix(x, y, k, n_hash, seeds)
    if m + n <= 3000:                     # R IS the matrix similarityMH_cross returns
        assert np.array_equal(bits(da.similarityMH_cross(x, y, k, n_hash, seed=SEED)), bits(R))
    if m == 130:
        assert -(-m // 128) * 128 + n > 131068 >= m + n
    s = session.MinHashSession(y, k, n_hash, seed=SEED, reserve=False)
    sub = np.arange(n - 1, -1, -3)
    for top in tops:
        assert_topk(da.similarityMH_cross_topk(x, y, k, n_hash, top, seed=SEED), R, top, ("mirror", m, n, top))
        assert_topk(host_mh(x, y, k, n_hash, seeds, top), R, top, ("host", m, n, top))
        assert_topk(device_mh(x, y, k, n_hash, seeds, top), R, top, ("one call", m, n, top))
        assert_topk(s.cross_topk(x, top), R, top, ("session", m, n, top))
        if top <= len(sub):
            assert_topk(s.cross_topk(x, top, sub), R[:, sub], top, ("session, subset", m, n, top))
    assert_topk(host_mh(x, y, k, n_hash, seeds, tops[0], with_val=False), R, tops[0], ("host, no values", m, n))
    # the mirror clamps top to len(y)
    if n <= 1024:
        assert_topk(da.similarityMH_cross_topk(x, y, k, n_hash, n + 7, seed=SEED), R, n, ("mirror, clamped", m, n))


def test_minhash_zero_columns_fill_a_row_and_no_forced_diagonal(da):
    x = ["ACDEFGHIK", "AC", "WWWWWWWW", "MMMMMMMMMM"]
    y = ["QQQQQQQQ", "AC", "ACDEFGHIK", "A", "ACDEFGHIR", "ACDEFGHIK"]
    R = mh_matrix(x, y, 4, 50, O.seeds(SEED, 50))
    idx, val = da.similarityMH_cross_topk(x, y, 4, 50, 4, seed=SEED)
    assert_topk((idx, val), R, 4, "small")
    assert idx[0].tolist()[:2] == [2, 5] and val[0, 0] == 1.0 and val[0, 1] == 1.0      # the string on both sides finds itself, twice, in order
    assert 0.0 < val[0, 2] < 1.0 and idx[0, 2] == 4
    assert idx[3].tolist() == [0, 1, 2, 3] and not val[3].any()                          # nothing in common: zeros fill the row, by position


def test_row_blocks_give_identical_results(da):
    m, n, k, n_hash, top = 300, 1000, 4, 500, 10
    x, y = two_sets(np.random.RandomState(77), m, n, "ACDEFGHIKLMNPQRSTVWY", high_bytes=True)
    seeds = O.seeds(SEED, n_hash)
    R = mh_matrix(x, y, k, n_hash, seeds)
    whole = (host_mh(x, y, k, n_hash, seeds, top), device_mh(x, y, k, n_hash, seeds, top))
    with switches(DYNAALIGN_BLOCK_BYTES=1024):                     # 128 rows: x is cut into three row blocks
        blocked = (host_mh(x, y, k, n_hash, seeds, top), device_mh(x, y, k, n_hash, seeds, top))
    for w, b in zip(whole, blocked):
        assert_topk(b, R, top, "blocked")
        assert np.array_equal(w[0], b[0]) and np.array_equal(bits(w[1]), bits(b[1]))
    xs, ys = nw_sets(np.random.RandomState(78), 260, 300)
    with switches(DYNAALIGN_BLOCK_BYTES=1024):
        nw_blocked = host_nw(xs, ys, "BLOSUM62", 10, 4, top)
    assert_topk(nw_blocked, nw_matrix(xs, ys, "BLOSUM62", 10, 4)[0], top, "NW, blocked")


# ---- da_dev_topk_rows alone ------------------------------------------------------------------------------------------------------------------

def run_topk_rows(keys, top, ld, offset, rank=None, rank_bits=0):
    from dynaalign_amd import device
    rows, n = keys.shape
    buf, view = strided(rows, n, ld, torch.int16, offset)
    view.copy_(torch.from_numpy(keys.view(np.int16)).cuda())
    rank_t = None if rank is None else torch.from_numpy(np.ascontiguousarray(rank, np.uint16).view(np.int16)).cuda()
    idx, key = device.topk_rows(view, top, rank_t, rank_bits)
    torch.cuda.synchronize()
    idx, key = idx.cpu().numpy(), key.cpu().numpy().view(np.uint16)
    r = (keys if rank is None else rank[keys]).astype(np.int64)
    want = np.argsort(-r, axis=1, kind="stable")[:, :top]
    bad = np.argwhere(idx != want)
    assert len(bad) == 0, ("topk_rows", keys.shape, top, ld, offset, bad[0].tolist(), idx[bad[0][0]][:12], want[bad[0][0]][:12])
    assert np.array_equal(key, np.take_along_axis(keys, want, axis=1))         # the KEY is returned, not its rank


def key_block(rng, rows, n, hi, zero_share=0.0):
    k = rng.randint(0, hi, (rows, n)).astype(np.uint16)
    if zero_share:
        k[rng.rand(rows, n) < zero_share] = 0
    return k


@pytest.mark.parametrize("n", [1, 7, 64, 777, 1024, 1025, 2048, 5000, 20001])
def test_topk_rows_layouts(da, n):
    rng = np.random.RandomState(n)
    keys = key_block(rng, 5, n, 40, zero_share=0.6)
    keys[1] = 123                                                   # a row of one repeated key
    keys[2] = 0
    keys[3] = (np.arange(n) % 65536).astype(np.uint16)              # increasing: the last columns win
    ld8 = -(-n // 8) * 8
    for top in sorted({1, min(n, 2), min(n, 10), min(n, 1024)}):
        for ld, offset in ((ld8, 0), (ld8 + 8, 8), (n + 1 - (n % 2), 0), (ld8, 3), (n, 1)):   # aligned, aligned, odd ld, unaligned base, both
            run_topk_rows(keys, top, ld, offset, rank_bits=16 if n > 40 else 0)
    run_topk_rows(key_block(rng, 3, n, 40), min(n, 10), ld8, 0, rank_bits=6)                  # one digit only


def test_topk_rows_rank_table_ties_distinct_keys(da):
    rng = np.random.RandomState(3)
    rank = (np.arange(65536) // 3).astype(np.uint16)                # three keys per rank
    for n, hi, bits_ in ((500, 30, 4), (3000, 2000, 10), (3000, 65536, 15), (1000, 65536, 0)):
        keys = key_block(rng, 4, n, hi, zero_share=0.3)
        assert len(np.unique(rank[keys[0]])) < len(np.unique(keys[0]))
        for top in (1, 10, min(n, 1024)):
            run_topk_rows(keys, top, -(-n // 8) * 8, 0, rank=rank, rank_bits=bits_)
            run_topk_rows(keys, top, n + 1, 5, rank=rank, rank_bits=bits_)
    # a table that maps EVERYTHING to one rank: the first columns, in order
    flat = np.full(65536, 9, np.uint16)
    run_topk_rows(key_block(rng, 2, 2500, 65536), 33, 2504, 0, rank=flat, rank_bits=4)


def test_topk_rows_top_equals_n_and_full_key_range(da):
    rng = np.random.RandomState(4)
    for n in (1, 2, 100, 1000, 1024):
        run_topk_rows(key_block(rng, 3, n, 65536), n, n, 0)
        run_topk_rows(key_block(rng, 3, n, 3), n, n + 3, 1, rank_bits=2)
    run_topk_rows(key_block(rng, 2000, 300, 501, zero_share=0.9), 10, 304, 0, rank_bits=9)     # many short rows: the one-wave form


# ---- NW ------------------------------------------------------------------------------------------------------------------------------------------

def nw_matrix(x, y, matrix, go, ge):
    m = len(x)
    rc, nm, ln, _, _ = O.nw_rows(x + y, 0, m, matrix, go, ge)
    assert rc == 0
    nm, ln = nm[:, m:], ln[:, m:]
    return nm.astype(np.float64) / ln.astype(np.float64), nm, ln


def nw_sets(rng, m, n):
    """lengths 1 .. 127 on both sides (two_sets' recipe without its empty strings), half of them short: small alignment lengths are where
    different (matches, length) pairs share a value"""
    x, y = two_sets(rng, m, n, AA24, 1, 128)
    short_x, short_y = two_sets(rng, m, n, "ACDW", 1, 9)
    x = [(b if i % 2 else a) or "W" for i, (a, b) in enumerate(zip(x, short_x))]
    y = [(b if j % 2 else a) or "W" for j, (a, b) in enumerate(zip(y, short_y))]
    return x, y


@pytest.mark.parametrize("matrix,go,ge,m,n", [("BLOSUM62", 10, 4, 150, 400), ("BLOSUM50", 11, 1, 129, 257), ("BLOSUM62", 10, 4, 40, 1100)])
def test_nw_against_the_oracle(da, matrix, go, ge, m, n):
    rng = np.random.RandomState(500 + m)
    x, y = nw_sets(rng, m, n)
    assert min(map(len, x + y)) >= 1 and 100 <= max(map(len, x + y)) <= 127
    R, nm, ln = nw_matrix(x, y, matrix, go, ge)
    assert np.array_equal(bits(da.similarityNW_cross(x, y, matrix, go, ge)), bits(R))            # R IS the matrix similarityNW_cross returns
    # the tie rule is really exercised: among the 10 best of some row there are columns of equal POSITIVE value and different codes,
    # and ordering by raw code would list them differently
    want_idx, want_val = expected(R, 10)
    code = (nm << 8) | ln
    sel = np.take_along_axis(code, want_idx, axis=1)
    tied = (want_val[:, 1:] == want_val[:, :-1]) & (sel[:, 1:] != sel[:, :-1]) & (want_val[:, 1:] > 0)
    assert int(tied.sum()) >= (5 if m >= 100 else 1), int(tied.sum())
    by_code = np.argsort(-code.astype(np.int64), axis=1, kind="stable")[:, :10]
    assert not np.array_equal(by_code, want_idx)
    for top in (1, 2, 10, min(n, 1024), n if n <= 1024 else 300):
        assert_topk(da.similarityNW_cross_topk(x, y, matrix, go, ge, top), R, top, ("NW mirror", matrix, top))
        assert_topk(host_nw(x, y, matrix, go, ge, top), R, top, ("NW host", matrix, top))
    if n <= 1024:
        assert_topk(da.similarityNW_cross_topk(x, y, matrix, go, ge, n + 5), R, n, ("NW mirror, clamped", matrix))


def test_nw_rank_table_on_the_device_equals_the_definition(da):
    """da_dev_topk_rows with the library's rank table on every code short sequences produce: the order of the doubles"""
    from dynaalign_amd import nw_code_ranks
    rank, distinct = nw_code_ranks(12)
    codes = np.array([(mt << 8) | ln for ln in range(1, 25) for mt in range(0, min(ln, 12) + 1)], np.uint16)
    rng = np.random.RandomState(8)
    keys = codes[rng.randint(0, len(codes), (6, 1500))]
    value = (keys >> 8).astype(np.float64) / (keys & 255).astype(np.float64)
    want = np.argsort(-value, axis=1, kind="stable")[:, :50]
    assert np.array_equal(np.argsort(-rank[keys].astype(np.int64), axis=1, kind="stable")[:, :50], want)
    run_topk_rows(keys, 50, 1504, 0, rank=rank, rank_bits=max(int(distinct - 1).bit_length(), 1))
