"""GPU tests of the exact Jaccard index for sequences of up to 1024 shingle positions: the device layer (device.jaccard_sets_long /
device.jaccard_rect_long), the host entry points (similarityJaccard_long, _cross_long, _cross_topk_long, _knn_long, _knn_edges_long,
_edges_long, _cross_edges_long, _stats_long) and clusterbreak on them.  The yardstick is the set definition, written here with Python sets
of byte slices -- independently of the package's jaccard_dense -- and every comparison is exact: indices and codes as integers, values as
uint64 bit patterns against Python's i / u."""
import functools
import io

import numpy as np
import pytest
import torch

from test_gpu_cross import bits, same, strided, switches
from test_gpu_jaccard import RECTS, as_bytes, edge_strings, family, quantile_type7_of, shingles
from test_stats_cpu import MEAN_RTOL, assert_stats

pytestmark = pytest.mark.gpu

AA20 = b"ACDEFGHIKLMNPQRSTVWY"
T = 64                      # tile edge of k_jaccard_rect_long
PACK32, F64 = 2, 0
POSITIONS = [0, 1, 63, 64, 65, 127, 128, 255, 256, 257, 1023, 1024]


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    from dynaalign_amd import _capi
    assert _capi.load().da_device_count() > 0
    return dynaalign_amd


# ---- inputs and the model ------------------------------------------------------------------------------------------------------------------

def rand_bytes(rng, length):
    return bytes(AA20[t] for t in rng.randint(0, 20, length))


def with_positions(rng, p, k):
    """a random string over 20 letters with p shingle positions at k (p = 0: one byte short of a shingle)"""
    return rand_bytes(rng, p + k - 1)


def long_family(rng, length, count):
    """`count` copies of one random parent of `length` residues with 0-5 substitutions and 0-2 indels each"""
    parent = rand_bytes(rng, length)
    out = []
    for _ in range(count):
        b = bytearray(parent)
        for _ in range(rng.randint(0, 6)):
            b[rng.randint(0, len(b))] = AA20[rng.randint(0, 20)]
        for _ in range(rng.randint(0, 3)):
            at = rng.randint(0, len(b))
            if rng.randint(0, 2):
                del b[at]
            else:
                b.insert(at, AA20[rng.randint(0, 20)])
        out.append(bytes(b))
    return parent, out


def long_edge_strings(rng, k):
    """the lists the kernels can get wrong: one key from 1024 positions, two keys, the all-ones key, the zero key, no key at all, 20 keys"""
    return [b"A" * 1024, b"A" * (1023 + k), b"AC" * 512, b"\xff" * 300, b"\x00" * 200 + b"\x01" + b"\x00" * 100, b"A" * (k - 1), b"",
            bytes(AA20[t] for t in rng.randint(0, 20, 1024)), b"\xff" * (k + 1) + b"\x00" * (k + 1)]


def model_counts(x, k, y=None):
    sx = [shingles(b, k) for b in x]
    if y is None:                                            # one set: the upper triangle, mirrored
        n = len(sx)
        inter = np.zeros((n, n), np.int64)
        for i in range(n):
            for j in range(i, n):
                inter[i, j] = inter[j, i] = len(sx[i] & sx[j])
        size = np.array([len(s) for s in sx], np.int64)
        return inter, size[:, None] + size[None, :] - inter
    sy = [shingles(b, k) for b in y]
    inter = np.array([[len(a & b) for b in sy] for a in sx], np.int64).reshape(len(sx), len(sy))
    union = np.array([[len(a | b) for b in sy] for a in sx], np.int64).reshape(len(sx), len(sy))
    return inter, union


def model_values(inter, union):
    """Python's divide of the two integers; 1.0 for two empty sets"""
    flat = [(int(i) / int(u)) if u else 1.0 for i, u in zip(inter.ravel().tolist(), union.ravel().tolist())]
    return np.array(flat, np.float64).reshape(inter.shape)


def model_codes(inter, union):
    return np.where(union > 0, inter << 16 | union, 1 << 16 | 1).astype(np.uint32)


class Data:
    def __init__(self, seqs, k):
        self.seqs, self.k = as_bytes(seqs), k
        self.inter, self.union = model_counts(self.seqs, k)
        self.J, self.codes = model_values(self.inter, self.union), model_codes(self.inter, self.union)
        self.n = len(self.seqs)
        for a in (self.inter, self.union, self.J, self.codes):
            a.setflags(write=False)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def device_sets(da, seqs, k):
    from dynaalign_amd import device
    res, off = da.pack_sequences(seqs)
    return device.jaccard_sets_long(device.DeviceSequences(res, off), k)


# ---- device layer: the sets ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 4, 5, 8])
def test_sets_are_the_sorted_distinct_shingles(da, k):
    rng = np.random.RandomState(100 + k)
    seqs = [with_positions(rng, p, k) for p in POSITIONS] + long_edge_strings(rng, k)
    if k == 1:
        assert len(shingles(seqs[-2], 1)) == 20 and len(seqs[-2]) == 1024             # 1024 positions, 20 keys
    sets = device_sets(da, seqs, k)
    torch.cuda.synchronize()
    keys = sets.keys.cpu().numpy().view(np.uint32 if k <= 4 else np.uint64)
    counts = sets.counts.cpu().numpy().view(np.uint16)
    most = max(len(b) for b in seqs) - k + 1
    assert most == 1024 and keys.dtype.itemsize == (4 if k <= 4 else 8) and sets.ld_keys == keys.shape[1] == 1024
    ones = (1 << (8 * k)) - 1
    seen_ones = seen_zero = False
    for i, b in enumerate(seqs):
        want = sorted(int.from_bytes(s, "big") for s in shingles(b, k))
        assert counts[i] == len(want), (i, len(b))
        assert keys[i, :len(want)].tolist() == want, (i, len(b))
        assert not keys[i, len(want):].any(), (i, len(b))
        seen_ones |= bool(want) and want[-1] == ones
        seen_zero |= bool(want) and want[0] == 0
    assert seen_ones and seen_zero                            # FF .. FF, the value a padded sort could mistake for a pad, and 0, the tail's value


def test_sets_ld_follows_the_longest_sequence(da):
    rng = np.random.RandomState(3)
    seqs = [with_positions(rng, p, 4) for p in (0, 5, 566, 130)] + [b"\xff" * 400]
    sets = device_sets(da, seqs, 4)
    torch.cuda.synchronize()
    assert sets.ld_keys == 568                                # 566 rounded up to 4
    keys, counts = sets.keys.cpu().numpy().view(np.uint32), sets.counts.cpu().numpy().view(np.uint16)
    for i, b in enumerate(seqs):
        want = sorted(int.from_bytes(s, "big") for s in shingles(b, 4))
        assert counts[i] == len(want) and keys[i, :len(want)].tolist() == want and not keys[i, len(want):].any()


# ---- device layer: the rectangle -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def rect_pool(k):
    """200 sequences, the model computed once per k: the lengths of POSITIONS and the edge strings mixed into three families of near-copies
    (300, 566 and 1000 residues), so that every 64-row tile holds lists of every kind"""
    rng = np.random.RandomState(40 + k)
    odd = [with_positions(rng, p, k) for p in POSITIONS] + long_edge_strings(rng, k)
    fam = [s for length, count in ((300, 60), (566, 60), (1000, 59)) for s in long_family(rng, length, count)[1]]
    order = rng.permutation(len(fam))
    seqs = [fam[t] for t in order]
    for t, s in enumerate(odd):                               # one odd string every ninth place, from the first place on
        seqs.insert(9 * t, s)
    seqs = seqs[:200]
    d = Data(seqs, k)
    # what the uint16 code of the short kernels cannot hold is present, and so are the empty sets
    assert d.n == 200 and (d.union > 255).any() and (d.inter > 127).any() and d.union.max() > 1500 and (d.union == 0).sum() >= 4
    off = d.inter[np.triu_indices(d.n, 1)]
    assert (off > 127).mean() > 0.2 and (off == 0).mean() > 0.05
    return d


@pytest.mark.parametrize("n", [1, 2, T - 1, T, T + 1, 2 * T + 1])
@pytest.mark.parametrize("k", [4, 5])
def test_rect_full_square_at_the_tile_edges(da, n, k):
    from dynaalign_amd import device
    d = rect_pool(k)
    sets = device_sets(da, d.seqs[:n], k)
    codes = device.jaccard_rect_long(sets, kind=PACK32)
    vals = device.jaccard_rect_long(sets, kind=F64)
    torch.cuda.synchronize()
    assert np.array_equal(u32(codes), d.codes[:n, :n])
    assert same(vals.cpu().numpy(), d.J[:n, :n])
    assert (d.codes[:n, :n] & 0xFFFF).min() >= 1
    if n > T:
        assert (d.union[:n, :n] > 255).any() and (d.inter[:n, :n] > 127).any()


@pytest.mark.parametrize("kind", [PACK32, F64], ids=["codes", "f64"])
def test_rect_odd_rectangles_odd_ld_and_offset_base(da, kind):
    """origins and extents that are no tile multiples, a single row, a single column, empty ranges, row and column ranges that overlap the
    diagonal, an odd leading dimension and a base one element into its allocation; what lies around the rectangle stays as it was"""
    from dynaalign_amd import _capi, device
    d = rect_pool(4)
    n = d.n
    sets = device_sets(da, d.seqs, 4)
    want_all = d.codes.view(np.int32) if kind == PACK32 else d.J
    dtype = torch.int32 if kind == PACK32 else torch.float64
    for r0, r1, c0, c1 in RECTS:
        rows, cols = r1 - r0, c1 - c0
        for ld, offset in ((cols, 0), (cols + 1 + cols % 2, 1), (cols + 8, 3)):      # the second: odd, whatever cols is
            buf, view = strided(max(rows, 1), max(cols, 1), max(ld, 1), dtype, offset)
            if rows and cols:
                device.jaccard_rect_long(sets, r0, r1, c0, c1, kind=kind, out=view)
            else:                                            # an empty rectangle is DA_OK and touches nothing
                _capi.check(_capi.load().da_dev_jaccard_rect_long(sets.keys.data_ptr(), sets.counts.data_ptr(), n, sets.ld_keys, 4, r0, r1, c0, c1,
                                                                  kind, view.data_ptr(), max(ld, 1), None))
            torch.cuda.synchronize()
            host = buf.cpu().numpy()
            want = np.full(host.shape, -7, host.dtype)
            if rows and cols:
                block = want_all[r0:r1, c0:c1]
                for r in range(rows):
                    want[offset + r * ld:offset + r * ld + cols] = block[r]
            if kind == PACK32:
                assert np.array_equal(host, want), (r0, r1, c0, c1, ld, offset)
            else:
                assert np.array_equal(host.view(np.uint64), want.view(np.uint64)), (r0, r1, c0, c1, ld, offset)


@pytest.mark.parametrize("k", [4, 5])
@pytest.mark.parametrize("kind", [PACK32, F64], ids=["codes", "f64"])
def test_symmetric_form_is_the_square_of_plain_rectangles(da, k, kind):
    """rows == columns launches the tiles on and above the diagonal and mirrors them; the same square put together from rectangles whose row
    and column ranges differ -- two off-diagonal blocks and the diagonal blocks in two column halves each -- is computed pair by pair"""
    from dynaalign_amd import device
    d = rect_pool(k)
    n, h = d.n, 100
    sets = device_sets(da, d.seqs, k)
    whole = device.jaccard_rect_long(sets, kind=kind)
    parts = torch.full_like(whole, -7)
    for r0, r1, c0, c1 in ((0, h, h, n), (h, n, 0, h), (0, h, 0, 37), (0, h, 37, h), (h, n, h, 165), (h, n, 165, n)):
        assert (r0, r1) != (c0, c1)
        device.jaccard_rect_long(sets, r0, r1, c0, c1, kind=kind, out=parts[r0:r1, c0:c1])
    torch.cuda.synchronize()
    a, b = whole.cpu().numpy(), parts.cpu().numpy()
    if kind == PACK32:
        assert np.array_equal(a, b) and np.array_equal(a.view(np.uint32), d.codes)
    else:
        assert same(a, b) and same(a, d.J)


# ---- host entry points ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=[4, 5], ids=["k4_u32", "k5_u64"])
def dl(request):
    """about 150 sequences, the model computed once per k: three families of near-copies of random parents of 300, 566 and 1000 residues, a
    dozen 20-mers cut from the parents, the edge strings and two byte-identical strings"""
    k = request.param
    rng = np.random.RandomState(7)
    seqs, parents = [], []
    for length, count in ((300, 70), (566, 35), (1000, 21)):
        parent, members = long_family(rng, length, count)
        parents.append(parent)
        seqs += members
    for t in range(12):
        p = parents[t % 3]
        at = rng.randint(0, len(p) - 20)
        seqs.append(p[at:at + 20])
    seqs += long_edge_strings(rng, k) + [b"A", b"AC", b"\x80\x81" * 30]               # the last one shares no shingle with any other
    seqs += [seqs[50], seqs[50]]                              # byte-identical to a family member and to each other
    order = rng.permutation(len(seqs))
    d = Data([seqs[t] for t in order], k)
    up = d.J[np.triu_indices(d.n, 1)]
    # a wrong all-zero result cannot pass what follows, and neither can the short kernels' uint16 code
    assert 140 <= d.n <= 160
    assert (up > 0).mean() >= 0.30 and len(np.unique(up)) >= 50 and np.quantile(up, 0.8) > 0
    assert np.diag(d.union).max() > 127 and (d.union > 255).any() and (d.inter > 127).any()
    assert (up == 1.0).sum() >= 3 and ((d.J > 0).sum(axis=1) == 1).any()               # ties at 1.0; a row that is zero off its diagonal
    return d


def blocks_of(cols, rows=40):
    """DYNAALIGN_BLOCK_BYTES that gives the rank paths blocks of `rows` rows of `cols` uint32 keys (the leading dimension is cols rounded up to 4)"""
    return rows * ((cols + 3) // 4 * 4) * 4


def both(run, cols, rows):
    """run() with the default block (one block) and cut into ceil(rows / 40) >= 3 row blocks: the same result"""
    run()
    assert rows > 80
    with switches(DYNAALIGN_BLOCK_BYTES=blocks_of(cols)):
        run()


def test_square_matrix(da, dl):
    got = da.similarityJaccard_long(dl.seqs, dl.k)
    assert same(got, dl.J)
    assert np.all(np.diag(got) == 1.0)


def test_square_matrix_in_three_row_blocks(da, dl):
    """the dense calls copy out blocks of at least 128 rows: the input twice is 3 blocks, and its model the model tiled (J[i, i] = 1.0 is also the
    value of the two copies of sequence i)"""
    twice = dl.seqs + dl.seqs
    assert len(twice) > 256
    with switches(DYNAALIGN_BLOCK_BYTES=1024):
        got = da.similarityJaccard_long(twice, dl.k)
    assert same(got, np.tile(dl.J, (2, 2)))


@pytest.mark.parametrize("column_major", [0, 1])
def test_cross_matrix_both_layouts(da, dl, column_major):
    from dynaalign_amd import _capi
    m = 77
    x, y = dl.seqs[:m], dl.seqs[m:]
    n = len(y)
    xr, xo = da.pack_sequences(x)
    yr, yo = da.pack_sequences(y)
    R = dl.J[:m, m:]
    out = np.full(m * n, -7.0)
    _capi.check(_capi.load().da_similarity_jaccard_cross_long(xr.ctypes.data, xo.ctypes.data, m, yr.ctypes.data, yo.ctypes.data, n, dl.k,
                                                              out.ctypes.data, column_major))
    assert same(out.reshape((n, m) if column_major else (m, n)), R.T if column_major else R)
    if not column_major:
        assert same(da.similarityJaccard_cross_long(x, y, dl.k), R)
        assert same(da.similarityJaccard_cross_long(y, x, dl.k), R.T)


@pytest.mark.parametrize("column_major", [0, 1])
def test_cross_matrix_in_three_row_blocks(da, dl, column_major):
    from dynaalign_amd import _capi
    x, y = dl.seqs + dl.seqs, dl.seqs[:70]
    if column_major:                                         # the blocks are rows of the transposed result: y is the long side
        x, y = y, x
    m, n = len(x), len(y)
    assert max(m, n) > 256
    R = np.tile(dl.J[:, :70], (2, 1))
    R = R.T if column_major else R
    xr, xo = da.pack_sequences(x)
    yr, yo = da.pack_sequences(y)
    out = np.full(m * n, -7.0)
    with switches(DYNAALIGN_BLOCK_BYTES=1024):
        _capi.check(_capi.load().da_similarity_jaccard_cross_long(xr.ctypes.data, xo.ctypes.data, m, yr.ctypes.data, yo.ctypes.data, n, dl.k,
                                                                  out.ctypes.data, column_major))
    assert same(out.reshape((n, m) if column_major else (m, n)), R.T if column_major else R)


def test_cross_topk(da, dl):
    m = 110
    x, y = dl.seqs[:m], dl.seqs[m - 30:]                   # thirty strings on both sides
    R = dl.J[:m, m - 30:]

    def run():
        for top in (1, 10, len(y) - 1):
            idx, val = da.similarityJaccard_cross_topk_long(x, y, dl.k, top)
            want = np.argsort(-R, axis=1, kind="stable")[:, :top]
            assert idx.dtype == np.int32 and np.array_equal(idx, want), top
            assert same(val, np.take_along_axis(R, want, axis=1)), top
    both(run, len(y), m)


def test_knn(da, dl):
    def run():
        for top in (1, 10, dl.n - 1):
            idx, val = da.similarityJaccard_knn_long(dl.seqs, dl.k, top)
            widx, wval = da.knn_dense(dl.J, top)
            assert idx.dtype == np.int32 and np.array_equal(idx, widx), top
            assert same(val, wval), top
    both(run, dl.n, dl.n)


@pytest.mark.parametrize("mode", ["union", "mutual"])
def test_knn_edges(da, dl, mode):
    thr, ei, ej, w = da.similarityJaccard_knn_edges_long(dl.seqs, dl.k, 10, mode)
    wi, wj, ww = da.knn_graph(*da.knn_dense(dl.J, 10), 1.0, mode)
    assert np.array_equal(ei, wi) and np.array_equal(ej, wj) and same(w, ww)
    off = ww[wi != wj]
    assert len(off) >= 100 and bits(thr) == bits(off.min())


@pytest.mark.parametrize("p", [0.0, 0.5, 0.8, 1.0])
def test_edges(da, dl, p):
    wthr = quantile_type7_of(dl.J[np.triu_indices(dl.n, 1)], p)
    wi, wj = np.nonzero(np.triu((dl.J >= wthr) & (dl.J > 0)))                          # row-major: sorted by (i, j)
    assert len(wi) > dl.n                                    # more than the diagonal

    def run():
        thr, ei, ej, w = da.similarityJaccard_edges_long(dl.seqs, dl.k, p)
        assert bits(thr) == bits(wthr), (thr, wthr)
        assert np.array_equal(ei, wi) and np.array_equal(ej, wj) and same(w, dl.J[wi, wj])
    both(run, dl.n, dl.n)
    if p == 0.8:
        assert wthr > 0


@pytest.mark.parametrize("form", ["absolute", "quantile"])
def test_cross_edges(da, dl, form):
    m = 100
    x, y = dl.seqs[:m], dl.seqs[m - 20:]
    R = dl.J[:m, m - 20:]
    cases = [0.0, 0.05, 0.5, 1.0, 1.5] if form == "absolute" else [0.0, 0.5, 0.8, 1.0]

    def run():
        for t in cases:
            if form == "absolute":
                thr, ei, ej, w = da.similarityJaccard_cross_edges_long(x, y, dl.k, threshold=t)
                wthr = t
            else:
                thr, ei, ej, w = da.similarityJaccard_cross_edges_long(x, y, dl.k, thresh_p=t)
                wthr = quantile_type7_of(R.ravel(), t)
            wi, wj = np.nonzero((R >= wthr) & (R > 0))
            assert bits(thr) == bits(wthr), (form, t, thr, wthr)
            assert np.array_equal(ei, wi) and np.array_equal(ej, wj) and same(w, R[wi, wj]), (form, t)
            assert t > 1.0 or len(wi) >= 20
    both(run, len(y), m)


def test_stats(da, dl):
    want = da.compute_similarity_stats(dl.J)

    def run():
        got = da.similarityJaccard_stats_long(dl.seqs, dl.k)
        assert_stats(got, dl.J)
        assert abs(got.mean_similarity - want.mean_similarity) <= MEAN_RTOL * abs(want.mean_similarity)
        assert tuple(got[4:]) == tuple(want[4:]) and [bits(v) for v in got[1:4]] == [bits(v) for v in want[1:4]]
    both(run, dl.n, dl.n)
    assert want.max_similarity == 1.0 and want.min_similarity == 0.0 and want.most_similar_pair == (0, 0)


def test_long_calls_on_short_sequences_are_the_short_calls(da):
    seqs = as_bytes(family(11, 3, 20, 120)) + edge_strings(4)
    n, m = len(seqs), 90
    x, y = seqs[:m], seqs[m - 10:]
    assert same(da.similarityJaccard_long(seqs, 4), da.similarityJaccard(seqs, 4))
    assert same(da.similarityJaccard_cross_long(x, y, 4), da.similarityJaccard_cross(x, y, 4))
    for top in (1, 10, n - 1):
        a, b = da.similarityJaccard_knn_long(seqs, 4, top), da.similarityJaccard_knn(seqs, 4, top)
        assert np.array_equal(a[0], b[0]) and same(a[1], b[1]), top
    for top in (1, 10, len(y)):
        a, b = da.similarityJaccard_cross_topk_long(x, y, 4, top), da.similarityJaccard_cross_topk(x, y, 4, top)
        assert np.array_equal(a[0], b[0]) and same(a[1], b[1]), top
    for p in (0.0, 0.8, 1.0):
        a, b = da.similarityJaccard_edges_long(seqs, 4, p), da.similarityJaccard_edges(seqs, 4, p)
        order = np.lexsort((b[2], b[1]))
        assert bits(a[0]) == bits(b[0]) and np.array_equal(a[1], b[1][order]) and np.array_equal(a[2], b[2][order]) and same(a[3], b[3][order]), p
    for mode in ("union", "mutual"):
        a, b = da.similarityJaccard_knn_edges_long(seqs, 4, 10, mode), da.similarityJaccard_knn_edges(seqs, 4, 10, mode)
        assert bits(a[0]) == bits(b[0]) and all(np.array_equal(u, v) for u, v in zip(a[1:3], b[1:3])) and same(a[3], b[3]), mode
    got = da.similarityJaccard_stats_long(seqs, 4)
    want = da.compute_similarity_stats(np.asarray(da.similarityJaccard(seqs, 4)))
    assert tuple(got[4:]) == tuple(want[4:]) and [bits(v) for v in got[1:4]] == [bits(v) for v in want[1:4]]
    assert abs(got.mean_similarity - want.mean_similarity) <= MEAN_RTOL * abs(want.mean_similarity)


def test_clusterbreak_on_the_edge_list_is_clusterbreak_on_the_dense_model(da):
    import importlib
    cb = importlib.import_module("dynaalign_amd.clusterbreak")
    rng = np.random.RandomState(31)
    pep = [s for _ in range(9) for s in long_family(rng, 300, 12)[1]] + [b"", b"A", b"AC", b"W" * 300, rand_bytes(rng, 566), rand_bytes(rng, 566)]
    pep = [b.decode("latin-1") for b in pep]
    kw = dict(size_max=10, size_min=3, log=io.StringIO())
    dense = cb.clusterbreak(pep, 0.8, sim_fn=lambda s: model_values(*model_counts(as_bytes(s), 4)), **kw)
    edges = cb.clusterbreak(pep, 0.8, edges_fn=lambda s: da.similarityJaccard_edges_long(s, k=4), **kw)
    assert np.array_equal(dense["clustered_seq"], edges["clustered_seq"]) and dense["filtered_seq"] == edges["filtered_seq"]
    assert dense.calls == edges.calls and dense.calls >= 3
    per_level = lambda res: [(lv["n"], np.float64(lv["threshold"]).view(np.uint64), lv["edges"]) for lv in res.levels]    # noqa: E731
    assert per_level(dense) == per_level(edges)
