"""GPU tests of the NW threshold forms for sequences of up to 1024 residues: similarityNW_edges_long / similarityNW_cross_edges_long on the host
boundary (the Python mirror and the raw C call), their row blocking, their agreement with the short calls, the device pieces on 32-bit keys
(da_dev_nw_codes_to_ranks, da_dev_rank_histogram, da_dev_threshold_ranks_*) against numpy, and clusterbreak(edges_fn=...) end to end.
Every expected value is built from the CPU oracle's matrix: the threshold is the library's (golden-pinned) quantile_type7 on np.unique's
merged values and counts, the edges are np.nonzero((R >= threshold) & (R > 0)) on the upper triangle with the diagonal or on the rectangle,
whose row-major order is the required order.  All comparisons are exact: i, j as integers, weight and threshold as uint64 bit patterns."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle_lib as O
from test_gpu_cross import AA24, bits, strided, switches  # noqa: F401
from test_gpu_cross_edges import assert_edges, expected, fetch, nw_threshold, thresh_kw
from test_gpu_topk import nw_sets

pytestmark = pytest.mark.gpu

AA20 = "ACDEFGHIKLMNPQRSTVWY"
QUANTILES = (0.0, 0.5, 0.8, 0.99, 1.0)
SQUARE_LENGTHS = (1, 5, 64, 65, 127, 128, 129, 255, 256, 257, 300)   # 128: past the short calls; 256+: past an 8-bit length; 65: the wavefront kernel


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    from dynaalign_amd import _capi
    assert _capi.load().da_device_count() > 0
    return dynaalign_amd


# ---- inputs and what the oracle says about them ----------------------------------------------------------------------------------------------

def rand_seq(rng, length, alphabet=AA20):
    return "".join(alphabet[t] for t in rng.randint(0, len(alphabet), length))


def mutate(rng, s, rate):
    """substitutions at `rate`, and now and then a residue dropped or doubled: relatives whose alignments have gaps"""
    out = []
    for ch in s:
        u = rng.rand()
        if u < rate:
            out.append(AA20[rng.randint(0, 20)])
        elif u < rate * 1.15:
            continue
        elif u < rate * 1.3:
            out.append(ch + ch)
        else:
            out.append(ch)
    return "".join(out)


def fit(rng, s, length):
    """exactly `length` residues: cut, or padded with random ones"""
    return s[:length] if len(s) >= length else s + rand_seq(rng, length - len(s))


@functools.lru_cache(maxsize=None)
def square_input():
    """44 sequences: every length of SQUARE_LENGTHS four times -- as mutated copies (5 .. 40 % substitutions) of three parents, so that the
    similarities spread from unrelated to near-identical, and once as an unrelated random string"""
    rng = np.random.RandomState(4242)
    parents = [rand_seq(rng, 320) for _ in range(3)]
    seqs = []
    for t, length in enumerate(SQUARE_LENGTHS):
        for c in range(3):
            seqs.append(fit(rng, mutate(rng, parents[(t + c) % 3], (0.05, 0.2, 0.4)[c]), length))
        seqs.append(rand_seq(rng, length))
    order = rng.permutation(len(seqs))
    return tuple(seqs[t] for t in order)


@functools.lru_cache(maxsize=None)
def far_input():
    """6 sequences at the far end: 1024 residues, a relative of 1000, a short one, a relative with deletions, and two unrelated long ones"""
    rng = np.random.RandomState(777)
    p = rand_seq(rng, 1024)
    return (p, fit(rng, mutate(rng, p, 0.1), 1000), rand_seq(rng, 17), mutate(rng, p[100:], 0.25)[:1024], rand_seq(rng, 1024), rand_seq(rng, 900))


@functools.lru_cache(maxsize=None)
def cross_input():
    """x (20) against y (50), 100 .. 300 residues: two families and unrelated strings, and the tie construction -- P (128) against P + Q
    (256) and P' (150) against P' + Q' (300) are both 0.5 from different (matches, length)"""
    rng = np.random.RandomState(9090)
    parents = [rand_seq(rng, 300) for _ in range(2)]
    P, Pp = rand_seq(rng, 128, "ACDEFGH"), rand_seq(rng, 150, "ACDEFGH")
    Q, Qp = rand_seq(rng, 128, "KLMNPQRS"), rand_seq(rng, 150, "KLMNPQRS")

    def member(t):
        length = int(rng.randint(100, 301))
        if t % 3 == 2:
            return rand_seq(rng, length)
        return fit(rng, mutate(rng, parents[t % 3], (0.03, 0.15, 0.35)[t % 3 + (t // 3) % 2]), length)
    x = [P, Pp] + [member(t) for t in range(18)]
    y = [P + Q, Pp + Qp] + [member(t) for t in range(48)]
    assert min(map(len, x + y)) >= 100 and max(map(len, x + y)) == 300
    return tuple(x), tuple(y)


@functools.lru_cache(maxsize=None)
def square_oracle(seqs, matrix, go, ge):
    """(R, matches, length) of similarityNW(seqs): the oracle runs once per input, whatever the number of thresholds and paths"""
    rc, R, msg = O.similarity_nw(list(seqs), matrix, go, ge)
    assert rc == 0, msg
    rc, nm, ln, _, msg = O.nw_rows(list(seqs), 0, len(seqs), matrix, go, ge)
    assert rc == 0, msg
    for a in (R, nm, ln):
        a.setflags(write=False)
    return R, nm, ln


@functools.lru_cache(maxsize=None)
def cross_oracle(x, y, matrix, go, ge):
    m = len(x)
    rc, nm, ln, _, msg = O.nw_rows(list(x) + list(y), 0, m, matrix, go, ge)
    assert rc == 0, msg
    nm, ln = nm[:, m:], ln[:, m:]
    R = nm.astype(np.float64) / ln.astype(np.float64)
    for a in (R, nm, ln):
        a.setflags(write=False)
    return R, nm, ln


def square_expected(R, p):
    """threshold <- quantile(R[upper.tri(R)], p); the edges: the upper triangle with the diagonal, R >= threshold and R > 0"""
    n = R.shape[0]
    thr = nw_threshold(R[np.triu_indices(n, 1)], p)
    mask = np.triu(np.ones((n, n), bool)) & (R >= thr) & (R > 0)
    i, j = np.nonzero(mask)
    return np.float64(thr), i.astype(np.int32), j.astype(np.int32), R[mask]


def host_square(seqs, matrix, go, ge, p):
    from dynaalign_amd import _capi
    lib = _capi.load()
    res, off = O.pack(list(seqs))
    h, thr, cnt = ctypes.c_void_p(), ctypes.c_double(-7.0), ctypes.c_int64(-7)
    _capi.check(lib.da_similarity_nw_edges_long_begin(res.ctypes.data, off.ctypes.data, len(seqs), matrix.encode(), go, ge, float(p),
                                                      ctypes.addressof(h), ctypes.addressof(thr), ctypes.addressof(cnt)))
    return fetch(lib, h, thr, cnt)


def host_cross(x, y, matrix, go, ge, thresh, is_q):
    from dynaalign_amd import _capi
    lib = _capi.load()
    xr, xo = O.pack(list(x))
    yr, yo = O.pack(list(y))
    h, thr, cnt = ctypes.c_void_p(), ctypes.c_double(-7.0), ctypes.c_int64(-7)
    _capi.check(lib.da_similarity_nw_cross_edges_long_begin(xr.ctypes.data, xo.ctypes.data, len(x), yr.ctypes.data, yo.ctypes.data, len(y),
                                                            matrix.encode(), go, ge, float(thresh), int(is_q), ctypes.addressof(h),
                                                            ctypes.addressof(thr), ctypes.addressof(cnt)))
    return fetch(lib, h, thr, cnt)


SCORING = [("BLOSUM62", 10, 4), ("BLOSUM50", 11, 1)]


# ---- 1. the square form ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("matrix,go,ge", SCORING, ids=[s[0] for s in SCORING])
def test_square_against_the_oracle(da, matrix, go, ge):
    seqs = square_input()
    assert sorted(set(map(len, seqs))) == list(SQUARE_LENGTHS) and len(seqs) == 44
    R, nm, ln = square_oracle(seqs, matrix, go, ge)
    iu = np.triu_indices(len(seqs), 1)
    assert ln[iu].max() > 255 and len(np.unique(R[iu])) > 300          # lengths past 8 bits; similarities that spread
    for p in QUANTILES:
        want = square_expected(R, p)
        assert len(want[1]) >= len(seqs)                                # the diagonal always survives
        if 0 < p < 1:
            assert len(want[1]) < int((np.triu(R) > 0).sum())
        assert_edges(da.similarityNW_edges_long(list(seqs), matrix, go, ge, p), want, ("mirror", matrix, p))
        assert_edges(host_square(seqs, matrix, go, ge, p), want, ("host", matrix, p))


# ---- 2. the far end --------------------------------------------------------------------------------------------------------------------------

def test_square_at_1024_residues(da):
    seqs = far_input()
    assert max(map(len, seqs)) == 1024 and 1000 in map(len, seqs) and min(map(len, seqs)) <= 20
    R, nm, ln = square_oracle(seqs, "BLOSUM62", 10, 4)
    iu = np.triu_indices(len(seqs), 1)
    assert ln[iu].max() > 1024 and nm[iu].max() > 800                   # alignment lengths past 1024; a rank near the top of the table
    for p in (0.5, 0.9):
        want = square_expected(R, p)
        assert len(seqs) < len(want[1]) < len(seqs) * (len(seqs) + 1) // 2
        assert_edges(da.similarityNW_edges_long(list(seqs), thresh_p=p), want, ("far end, mirror", p))
        assert_edges(host_square(seqs, "BLOSUM62", 10, 4, p), want, ("far end, host", p))


# ---- 3. the two-set form ---------------------------------------------------------------------------------------------------------------------

CROSS_FORMS = [(0.5, 1), (0.9, 1), (0.99, 1), (-1.0, 0), (0.0, 0), (0.5, 0), (None, 0), (2.0, 0)]   # None: a value R takes, see below


def cross_forms(R):
    taken = np.sort(R[R > 0])
    v = float(taken[(3 * len(taken)) // 4])                             # computed with numpy's divide in cross_oracle: the >= boundary
    return [(v if t is None else t, q) for t, q in CROSS_FORMS]


def test_the_cross_input_meets_the_conditions_it_is_built_for():
    """so that the comparisons below cannot pass vacuously (figures: the oracle's)"""
    x, y = cross_input()
    assert (len(x), len(y)) == (20, 50)
    R, nm, ln = cross_oracle(x, y, "BLOSUM62", 10, 4)
    assert (nm[0, 0], ln[0, 0]) == (128, 256) and (nm[1, 1], ln[1, 1]) == (150, 300)
    want = expected(R, 0.5)
    kept_half = want[3] == 0.5
    codes = {(int(nm[i, j]), int(ln[i, j])) for i, j in zip(want[1][kept_half], want[2][kept_half])}
    assert len(codes) >= 2 and {(128, 256), (150, 300)} <= codes        # different codes of one value among the kept edges
    thr = nw_threshold(R, 0.99)
    _, i, j, w = expected(R, thr)
    assert 0 < len(i) < int((R > 0).sum()) and R[R > 0].min() < thr < R.max()
    assert int((np.bincount(i, minlength=len(x)) == 0).sum()) > 0       # a row without any edge
    assert len(expected(R, 2.0)[1]) == 0 and len(expected(R, -1.0)[1]) == int((nm > 0).sum())


@pytest.mark.parametrize("matrix,go,ge", SCORING, ids=[s[0] for s in SCORING])
def test_cross_against_the_oracle(da, matrix, go, ge):
    x, y = cross_input()
    R, nm, ln = cross_oracle(x, y, matrix, go, ge)
    for thresh, is_q in cross_forms(R):
        want = expected(R, nw_threshold(R, thresh) if is_q else thresh)
        what = (matrix, thresh, "quantile" if is_q else "absolute")
        assert_edges(da.similarityNW_cross_edges_long(list(x), list(y), matrix, go, ge, **thresh_kw(thresh, is_q)), want, ("mirror",) + what)
        assert_edges(host_cross(x, y, matrix, go, ge, thresh, is_q), want, ("host",) + what)


# ---- 4. row blocks ---------------------------------------------------------------------------------------------------------------------------

def test_row_blocks_give_identical_results(da):
    seqs = square_input()
    x, y = cross_input()
    R = square_oracle(seqs, "BLOSUM62", 10, 4)[0]
    Rc = cross_oracle(x, y, "BLOSUM62", 10, 4)[0]
    for p in (0.0, 0.8, 0.99):
        whole = host_square(seqs, "BLOSUM62", 10, 4, p)
        with switches(DYNAALIGN_BLOCK_BYTES=1500):                     # 44 columns of 4 bytes: 8 rows a block, 6 blocks; the DP runs twice
            blocked = host_square(seqs, "BLOSUM62", 10, 4, p)
            mirror = da.similarityNW_edges_long(list(seqs), thresh_p=p)
        assert_edges(blocked, square_expected(R, p), ("square, blocked", p))
        assert_edges(mirror, whole, ("square, mirror blocked against whole", p))
    for thresh, is_q in cross_forms(Rc):
        whole = host_cross(x, y, "BLOSUM62", 10, 4, thresh, is_q)
        with switches(DYNAALIGN_BLOCK_BYTES=1700):                     # 52 keys a row: 8 rows a block, 3 blocks
            blocked = host_cross(x, y, "BLOSUM62", 10, 4, thresh, is_q)
        assert_edges(blocked, expected(Rc, nw_threshold(Rc, thresh) if is_q else thresh), ("cross, blocked", thresh, is_q))
        assert_edges(blocked, whole, ("cross, blocked against whole", thresh, is_q))


# ---- 5. continuity with the short calls ------------------------------------------------------------------------------------------------------

def test_short_inputs_give_what_the_short_calls_give(da):
    x, y = nw_sets(np.random.RandomState(31), 40, 90)
    assert max(map(len, x + y)) <= 127
    for p in QUANTILES:
        assert_edges(da.similarityNW_edges_long(y, thresh_p=p), tuple(map(np.asarray, da.similarityNW_edges(y, thresh_p=p))), ("square", p))
    for thresh, is_q in ((0.5, 1), (0.9, 1), (1.0, 1), (-1.0, 0), (0.5, 0), (2.0, 0)):
        kw = thresh_kw(thresh, is_q)
        assert_edges(da.similarityNW_cross_edges_long(x, y, **kw), tuple(map(np.asarray, da.similarityNW_cross_edges(x, y, **kw))), ("cross", kw))


# ---- 6. the pieces alone -----------------------------------------------------------------------------------------------------------------------

def u32(t):
    return t.cpu().numpy().view(np.uint32)


def rank_layouts(n):
    ld4 = -(-n // 4) * 4
    return ((ld4, 0), (ld4 + 4, 4), (n + 1 - (n % 2), 0), (ld4, 1), (n, 3))        # aligned; aligned, offset; odd ld; base off by 1; by 3


def run_rank_pieces(keys, nbins, r_min, ld, offset, tri, row_begin, col_begin):
    """histogram, count + emit (sized from the count, then sentinel-filled buffers at capacities around the total) of one block of uint32 keys
    in one layout and one mask mode, against numpy"""
    from dynaalign_amd import _capi, device
    lib = _capi.load()
    rows, n = keys.shape
    buf, view = strided(rows, n, ld, torch.int32, offset)
    view.copy_(torch.from_numpy(keys.view(np.int32)).cuda())
    what = (keys.shape, nbins, r_min, ld, offset, tri, row_begin, col_begin)
    grow, gcol = row_begin + np.arange(rows)[:, None], col_begin + np.arange(n)[None, :]
    inside = keys < nbins
    counted = inside & ((gcol > grow) if tri else True)
    hist = device.rank_histogram(view, nbins, tri, row_begin, col_begin).cpu().numpy()
    assert np.array_equal(hist, np.bincount(keys[counted].ravel(), minlength=nbins)), ("histogram",) + what
    flag = inside & (keys >= r_min) & ((gcol >= grow) if tri else True)
    wi, wj = np.nonzero(flag)
    wkey = keys[flag]
    want_ptr = np.searchsorted(wi, np.arange(rows + 1))
    rowptr, j, key = device.threshold_ranks(view, r_min, nbins, tri, row_begin, col_begin)
    torch.cuda.synchronize()
    assert np.array_equal(rowptr.cpu().numpy(), want_ptr), ("row pointers",) + what
    assert np.array_equal(j.cpu().numpy(), wj) and np.array_equal(u32(key), wkey), ("emit",) + what
    total = len(wj)
    for cap in sorted({0, total // 2, total, total + 9}):
        dj = torch.full((total + 16,), -7, dtype=torch.int32, device="cuda")
        dk = torch.full((total + 16,), -7, dtype=torch.int32, device="cuda")
        _capi.check(lib.da_dev_threshold_ranks_emit(view.data_ptr(), rows, n, ld, r_min, nbins, int(tri), row_begin, col_begin, rowptr.data_ptr(),
                                                    dj.data_ptr(), dk.data_ptr(), cap, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        stored = min(cap, total)
        assert np.array_equal(dj[:stored].cpu().numpy(), wj[:stored]) and np.array_equal(u32(dk[:stored]), wkey[:stored]), ("emit, capacity", cap) + what
        assert bool((dj[stored:] == -7).all()) and bool((dk[stored:] == -7).all()), ("written beyond the capacity or the total", cap) + what
    # the key block is only read: the sentinel fill around and between its rows is intact, and so are the keys
    pad = torch.ones(buf.numel(), dtype=torch.bool, device="cuda")
    torch.as_strided(pad, (rows, n), (ld, 1), offset).fill_(False)
    assert bool((buf[pad] == -7).all()) and np.array_equal(u32(view.contiguous()), keys)


def rank_block(rng, n, nbins, hot):
    """7 rows: 60 % one hot key (the contended case) among random keys, some beyond nbins; all kept; none kept; only the last column kept;
    random again; all one key beyond nbins; 60 % rank 0"""
    hi = nbins + max(nbins // 8, 3)
    keys = rng.randint(0, hi, (7, n)).astype(np.uint32)
    keys[0][rng.rand(n) < 0.6] = hot
    keys[1] = nbins - 1                                             # all kept
    keys[2] = 0                                                     # none kept (r_min >= 1)
    keys[3] = 0
    keys[3, -1] = nbins - 1                                         # only the last column
    keys[5] = hi + 5                                                # neither counted nor kept
    keys[6][rng.rand(n) < 0.6] = 0
    return keys


@pytest.mark.parametrize("n", [1, 7, 64, 777, 2049])
def test_pieces_layouts_and_mask_modes(da, n):
    rng = np.random.RandomState(100 + n)
    for nbins in (2, 8193, 1300000):
        hot = nbins // 3
        keys = rank_block(rng, n, nbins, hot)
        if n >= 64:
            assert (keys >= nbins).any() and (keys[0] == hot).mean() > 0.5
        r_min = max(1, nbins // 2)
        for ld, offset in rank_layouts(n):
            run_rank_pieces(keys, nbins, r_min, ld, offset, False, 0, 0)
            # the diagonal through the middle of the block: rows 3 .. 9 below the block's first global column + n // 2
            run_rank_pieces(keys, nbins, r_min, ld, offset, True, 10 + n // 2 - 3, 10)
        run_rank_pieces(keys, nbins, 1, n, 0, False, 0, 0)          # every positive rank kept
        run_rank_pieces(keys, nbins, 1, n, 0, True, 0, 0)           # the block at the origin of the square
        run_rank_pieces(keys, nbins, 1, n, 0, True, n + 20, 0)      # entirely below the diagonal: nothing counted, nothing kept
        run_rank_pieces(keys, nbins, nbins, n, 0, False, 0, 0)      # a threshold above every value


def test_pieces_many_rows_and_a_hot_key(da):
    """300 rows of 777 keys, 60 % on one rank and most of the rest on a handful: every workgroup of the histogram meets the hot bins; and the
    one-wave / four-wave forms of count and emit at 1024 / 1025 columns"""
    rng = np.random.RandomState(12)
    nbins = 1300000
    few = rng.randint(1, nbins, 6).astype(np.uint32)
    keys = few[rng.randint(0, 6, (300, 777))]
    keys[rng.rand(300, 777) < 0.6] = 987654
    rare = rng.rand(300, 777) < 0.05
    keys[rare] = rng.randint(0, nbins + 1000, int(rare.sum())).astype(np.uint32)
    keys[17] = 0                                                    # a row without any edge
    run_rank_pieces(keys, nbins, 900000, 780, 0, False, 0, 0)
    run_rank_pieces(keys, nbins, 900000, 777, 3, True, 200, 0)
    zeros = keys.copy()
    zeros[rng.rand(300, 777) < 0.9] = 0                             # mostly rank 0
    run_rank_pieces(zeros, nbins, 1, 780, 0, True, 0, 100)
    for n in (1024, 1025):
        keys = rng.randint(0, 5000, (40, n)).astype(np.uint32)
        run_rank_pieces(keys, 4000, 2000, n + 4 - n % 4, 0, False, 0, 0)
        run_rank_pieces(keys, 4000, 2000, n + 4 - n % 4, 0, True, 500, 0)


@pytest.mark.parametrize("n", [1, 1024, 1025])
def test_pieces_the_16_bit_and_the_32_bit_instantiation_agree(da, n):
    """One block of keys below 65 536 through da_dev_threshold_rows_count / _emit as uint16 with keep[v] = (v >= r_min) and through
    da_dev_threshold_ranks_count / _emit as uint32 (rectangle, the same r_min): the same row pointers, columns and keys, element for element.
    n = 1: a lone tail; 1024 / 1025: the two sides of the one-wave / 256-thread switch.  ld = n + 3 and a base one key into the allocation put
    rows off the 16-byte boundary (the single-key loads); the capacity is one below the total, so the last slot stays as it was."""
    from dynaalign_amd import _capi, device
    lib = _capi.load()
    rng = np.random.RandomState(500 + n)
    rows, ld, nbins, r_min = 3, n + 3, 65536, 40000
    keys = rng.randint(0, nbins, (rows, n)).astype(np.uint32)
    keys[rng.rand(rows, n) < 0.3] = 0                               # key 0: the 16-bit form decides it from a register
    keys[:, -1] = nbins - 1 - np.arange(rows)                       # every row keeps its last column: the total is at least 3
    keep = (np.arange(nbins) >= r_min).astype(np.uint8)
    _, v16 = strided(rows, n, ld, torch.int16, 1)
    _, v32 = strided(rows, n, ld, torch.int32, 1)
    v16.copy_(torch.from_numpy(keys.astype(np.uint16).view(np.int16)).cuda())
    v32.copy_(torch.from_numpy(keys.view(np.int32)).cuda())
    keep_t = torch.from_numpy(keep).cuda()
    p16, j16, k16 = device.threshold_rows(v16, keep_t)
    p32, j32, k32 = device.threshold_ranks(v32, r_min, nbins)
    torch.cuda.synchronize()
    want_ptr = np.concatenate([[0], np.cumsum((keys >= r_min).sum(axis=1))])
    total = int(want_ptr[-1])
    assert total >= 3
    want_j, want_key = np.nonzero(keys >= r_min)[1], keys[keys >= r_min]      # row-major: rows ascending, columns ascending within a row
    assert np.array_equal(p16.cpu().numpy(), want_ptr) and np.array_equal(p32.cpu().numpy(), want_ptr)
    assert np.array_equal(j16.cpu().numpy(), j32.cpu().numpy()) and np.array_equal(j32.cpu().numpy(), want_j)
    assert np.array_equal(k16.cpu().numpy().view(np.uint16).astype(np.uint32), u32(k32)) and np.array_equal(u32(k32), want_key)
    stream = torch.cuda.current_stream().cuda_stream
    dj16, dj32, dk32 = (torch.full((total + 4,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    dk16 = torch.full((total + 4,), -7, dtype=torch.int16, device="cuda")
    _capi.check(lib.da_dev_threshold_rows_emit(v16.data_ptr(), rows, n, ld, keep_t.data_ptr(), nbins, p16.data_ptr(), dj16.data_ptr(), dk16.data_ptr(),
                                               total - 1, stream))
    _capi.check(lib.da_dev_threshold_ranks_emit(v32.data_ptr(), rows, n, ld, r_min, nbins, 0, 0, 0, p32.data_ptr(), dj32.data_ptr(), dk32.data_ptr(),
                                                total - 1, stream))
    torch.cuda.synchronize()
    assert np.array_equal(dj16.cpu().numpy(), dj32.cpu().numpy())   # the sentinels behind the capacity included
    assert np.array_equal(dj16[:total - 1].cpu().numpy(), j16[:total - 1].cpu().numpy())
    assert np.array_equal(dk16[:total - 1].cpu().numpy().view(np.uint16).astype(np.uint32), u32(dk32[:total - 1]))
    assert np.array_equal(dk16[:total - 1].cpu().numpy(), k16[:total - 1].cpu().numpy())
    assert bool((dj16[total - 1:] == -7).all()) and bool((dk16[total - 1:] == -7).all()) and bool((dk32[total - 1:] == -7).all())


@pytest.mark.parametrize("max_len", [3, 127, 1024])
def test_codes_to_ranks_against_the_host_table(da, max_len):
    from dynaalign_amd import device, nw_value_ranks
    values, rank = nw_value_ranks(max_len)
    rng = np.random.RandomState(max_len)
    rows, n = 9, 1301
    ln = rng.randint(1, 2 * max_len + 1, (rows, n))
    mt = np.minimum(rng.randint(0, max_len + 1, (rows, n)), ln)
    ln[0, :4], mt[0, :4] = (2 * max_len, 2 * max_len, 1, max_len), (max_len, 0, 1, max_len)        # the corners of the domain
    codes = ((mt.astype(np.uint32) << 16) | ln.astype(np.uint32))
    want = rank[ln, mt]
    # outside the domain: length 0, length > 2 * max_len, matches > max_len, matches > length, all bits set -- rank 0, and nothing is read
    outside = np.array([0, 5 << 16, 2 * max_len + 1, 0xFFFF, ((max_len + 1) << 16) | (2 * max_len), (2 << 16) | 1, 0xFFFFFFFF, 0xFFFF0001],
                       np.uint32)
    codes[1, :len(outside)] = outside
    want[1, :len(outside)] = 0
    rank_t = torch.from_numpy(rank.view(np.int32).ravel().copy()).cuda()
    for ld, offset in ((1304, 0), (1303, 1)):
        buf, view = strided(rows, n, ld, torch.int32, offset)
        view.copy_(torch.from_numpy(codes.view(np.int32)).cuda())
        out = device.nw_codes_to_ranks(view, rank_t, max_len)
        torch.cuda.synchronize()
        assert np.array_equal(u32(out), want) and np.array_equal(u32(view.contiguous()), codes)
        assert device.nw_codes_to_ranks(view, rank_t, max_len, out=view) is view                   # in place
        torch.cuda.synchronize()
        assert np.array_equal(u32(view.contiguous()), want)
        pad = torch.ones(buf.numel(), dtype=torch.bool, device="cuda")
        torch.as_strided(pad, (rows, n), (ld, 1), offset).fill_(False)
        assert bool((buf[pad] == -7).all())
    assert np.array_equal(values[want[0]].view(np.uint64), (mt[0] / ln[0]).view(np.uint64))       # values[rank] is the divide, bit for bit


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------------------

def test_clusterbreak_on_the_long_edge_list_and_consensus(da):
    rng = np.random.RandomState(2024)
    parents = [rand_seq(rng, 200) for _ in range(3)]
    pep = [fit(rng, mutate(rng, parents[t % 3], 0.04 + 0.02 * (t % 5)), int(rng.randint(130, 201))) for t in range(60)]
    assert min(map(len, pep)) >= 130 and max(map(len, pep)) <= 200
    p = 0.8
    dense = da.clusterbreak(pep, p, sim_fn=lambda s: da.similarityNW(s))
    edges = da.clusterbreak(pep, p, edges_fn=lambda s: da.similarityNW_edges_long(s, thresh_p=p))
    assert np.array_equal(dense["clustered_seq"], edges["clustered_seq"]) and dense["filtered_seq"] == edges["filtered_seq"]
    assert dense.calls == edges.calls and len(dense.levels) == len(edges.levels) >= 1
    for a, b in zip(dense.levels, edges.levels):
        assert (a["itr"], a["n"], a["edges"], a["clusters"]) == (b["itr"], b["n"], b["edges"], b["clusters"])
        assert np.array_equal(bits(np.float64(a["threshold"])), bits(np.float64(b["threshold"])))
    rows = edges["clustered_seq"]
    assert len(rows) > 0
    cons = da.clusterconsensus(rows, align_fn=da.nw_align_long)
    ids = list(dict.fromkeys(r[1] for r in rows))
    assert [c[0] for c in cons] == ids and all(isinstance(c[1], str) and len(c[1]) >= 100 for c in cons)
