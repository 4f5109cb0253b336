"""GPU tests of the exact Jaccard index of k-shingle sets: the device layer (device.jaccard_sets / device.jaccard_rect), the host entry points
(similarityJaccard, _cross, _cross_topk, _knn, _knn_edges, _edges) and clusterbreak on them.  The yardstick is the set definition, written here
with Python sets of byte slices -- independently of the package's jaccard_dense -- and every comparison is exact: indices and codes as integers,
values as uint64 bit patterns."""
import io

import numpy as np
import pytest
import torch

from test_gpu_cross import bits, same, strided, switches

pytestmark = pytest.mark.gpu

AA20 = "ACDEFGHIKLMNPQRSTVWY"
T = 64                      # tile edge of k_jaccard_rect
COMPACT, F64 = 1, 0
RATIO = np.array([[(i / u) if u else 1.0 for u in range(255)] for i in range(128)])      # Python's divide of the two integers; 1.0 at union 0


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    from dynaalign_amd import _capi
    assert _capi.load().da_device_count() > 0
    return dynaalign_amd


def family(seed, parents, length, count):
    """`count` strings: a random one of `parents` random strings over the 20 amino-acid letters with 0-3 substitutions and, half the time, one
    residue dropped at the front or appended at the back"""
    rng = np.random.RandomState(seed)
    par = ["".join(AA20[t] for t in rng.randint(0, 20, length)) for _ in range(parents)]
    out = []
    for _ in range(count):
        s = list(par[rng.randint(0, parents)])
        for _ in range(rng.randint(0, 4)):
            s[rng.randint(0, len(s))] = AA20[rng.randint(0, 20)]
        s = "".join(s)
        if rng.randint(0, 2):
            s = s[1:] if rng.randint(0, 2) else s + AA20[rng.randint(0, 20)]
        out.append(s)
    return out


def edge_strings(k):
    return [b"", b"A", b"AC", b"ACDEFGHI"[:k], b"W" * 20, b"ACDEFGHIKLMNPQRSTV\x80", b"ACDEFGHIKLMNPQR\xe9\xff", b"AC\xff\xff\xff\xffDEFGHIKLMN",
            b"ACDEFGHIKLMNPQRSTVWY", b"ACDEFGHIKLMNPQRSTVWY"]


def as_bytes(seqs):
    return [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in seqs]


def shingles(b, k):
    return {b[p:p + k] for p in range(len(b) - k + 1)}


def model_counts(x, k, y=None):
    sx = [shingles(b, k) for b in as_bytes(x)]
    sy = sx if y is None else [shingles(b, k) for b in as_bytes(y)]
    inter = np.array([[len(a & b) for b in sy] for a in sx], np.int64).reshape(len(sx), len(sy))
    union = np.array([[len(a | b) for b in sy] for a in sx], np.int64).reshape(len(sx), len(sy))
    return inter, union


def model_values(inter, union):
    return RATIO[inter, union]


def model_codes(inter, union):
    return np.where(union > 0, inter << 8 | union, 0x0101).astype(np.uint16)


def u16(t):
    return t.cpu().numpy().view(np.uint16)


class Data:
    def __init__(self, seqs, k):
        self.seqs, self.k = as_bytes(seqs), k
        self.inter, self.union = model_counts(self.seqs, k)
        self.J, self.codes = model_values(self.inter, self.union), model_codes(self.inter, self.union)
        self.n = len(self.seqs)


@pytest.fixture(scope="module")
def d4():
    """300 20-mers of 3 families + the edge strings, k = 4: the input of the host-boundary tests, its model computed once"""
    d = Data(family(11, 3, 20, 300) + edge_strings(4), 4)
    up = d.J[np.triu_indices(d.n, 1)]
    # a wrong all-zero result cannot pass what follows
    assert (up > 0).mean() >= 0.30 and len(np.unique(up)) >= 50 and np.quantile(up, 0.8) > 0
    return d


def device_sets(da, seqs, k):
    from dynaalign_amd import device
    res, off = da.pack_sequences(seqs)
    return device.jaccard_sets(device.DeviceSequences(res, off), k)


# ---- device layer ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 4, 5, 8])
def test_sets_are_the_sorted_distinct_shingles(da, k):
    seqs = as_bytes(family(3, 3, 20, 70)) + edge_strings(k) + [b"\xff" * 11, b"\x00" * 9 + b"\x01", b"BA" * 10]
    sets = device_sets(da, seqs, k)
    torch.cuda.synchronize()
    keys = sets.keys.cpu().numpy().view(np.uint32 if k <= 4 else np.uint64)
    counts = sets.counts.cpu().numpy()
    most = max(len(b) for b in seqs) - k + 1
    assert keys.dtype.itemsize == (4 if k <= 4 else 8) and sets.ld_keys == keys.shape[1] == (most + 3) // 4 * 4
    for i, b in enumerate(seqs):
        want = sorted(int.from_bytes(s, "big") for s in shingles(b, k))
        assert counts[i] == len(want), (i, b)
        assert keys[i, :len(want)].tolist() == want, (i, b)
        assert not keys[i, len(want):].any(), (i, b)


@pytest.mark.parametrize("n", [1, 2, T - 1, T, T + 1, 2 * T + 1])
@pytest.mark.parametrize("k", [4, 5])
def test_rect_full_square_at_the_tile_edges(da, n, k):
    from dynaalign_amd import device
    seqs = (edge_strings(k)[:min(n, 6)] + as_bytes(family(5, 3, 20, n)))[:n]
    d = Data(seqs, k)
    sets = device_sets(da, seqs, k)
    codes = device.jaccard_rect(sets, kind=COMPACT)
    vals = device.jaccard_rect(sets, kind=F64)
    torch.cuda.synchronize()
    assert np.array_equal(u16(codes), d.codes)
    assert same(vals.cpu().numpy(), d.J)
    assert (d.codes & 0xFF).min() >= 1


RECTS = [(0, 1, 0, 1), (5, 70, 3, 131), (63, 66, 0, 200), (0, 200, 64, 65), (1, 130, 1, 130), (100, 197, 37, 180), (37, 180, 100, 197),
         (128, 200, 0, 128), (7, 7, 0, 200), (0, 200, 9, 9)]


@pytest.mark.parametrize("kind", [COMPACT, F64], ids=["codes", "f64"])
def test_rect_odd_rectangles_odd_ld_and_offset_base(da, d4, kind):
    """origins and extents that are no tile multiples, row and column ranges that overlap the diagonal, an odd leading dimension and a base
    one element into its allocation; what lies around the rectangle stays as it was"""
    from dynaalign_amd import device
    n = 200
    sets = device_sets(da, d4.seqs[d4.n - n:], 4)        # the edge strings are among them
    lo = d4.n - n
    want_all = d4.codes if kind == COMPACT else d4.J
    dtype = torch.int16 if kind == COMPACT else torch.float64
    for r0, r1, c0, c1 in RECTS:
        rows, cols = r1 - r0, c1 - c0
        for ld, offset in ((cols, 0), (cols + 1 + cols % 2, 1), (cols + 8, 3)):      # the second: odd, whatever cols is
            buf, view = strided(max(rows, 1), max(cols, 1), max(ld, 1), dtype, offset)
            if rows and cols:
                device.jaccard_rect(sets, r0, r1, c0, c1, kind=kind, out=view)
            else:                                            # an empty rectangle is DA_OK and touches nothing
                from dynaalign_amd import _capi
                _capi.check(_capi.load().da_dev_jaccard_rect(sets.keys.data_ptr(), sets.counts.data_ptr(), n, sets.ld_keys, 4, r0, r1, c0, c1, kind,
                                                             view.data_ptr(), max(ld, 1), None))
            torch.cuda.synchronize()
            host = buf.cpu().numpy()
            want = np.full(host.shape, -7, host.dtype)
            if rows and cols:
                block = want_all[lo + r0:lo + r1, lo + c0:lo + c1]
                block = block.view(np.int16) if kind == COMPACT else block
                for r in range(rows):
                    want[offset + r * ld:offset + r * ld + cols] = block[r]
            if kind == COMPACT:
                assert np.array_equal(host, want), (r0, r1, c0, c1, ld, offset)
            else:
                assert np.array_equal(host.view(np.uint64), want.view(np.uint64)), (r0, r1, c0, c1, ld, offset)


def sequences_of_127_shingles(length):
    """70 strings of `length` upper-case letters in 3 families with 0-3 substitutions each, and 14 strings without any shingle among them"""
    rng = np.random.RandomState(21)
    par = [bytes(rng.randint(65, 91, length).astype(np.uint8)) for _ in range(3)]
    seqs = []
    for t in range(70):
        b = bytearray(par[t % 3])
        for _ in range(t % 4):
            b[rng.randint(0, length)] = rng.randint(97, 123)          # lower case: a substitution never repeats a shingle of the parent
        seqs.append(bytes(b))
        if t % 5 == 0:
            seqs.append(b"" if t % 10 else b"AC")
    return seqs


@pytest.mark.parametrize("k,length", [(4, 130), (8, 134)], ids=["k4_u32", "k8_u64"])
def test_rect_127_shingles_beside_empty_sets(da, k, length):
    """every non-empty sequence has 127 distinct shingles -- the longest list, the largest union (254), the largest LDS tile -- and shares its
    tiles with empty sets"""
    from dynaalign_amd import device
    seqs = sequences_of_127_shingles(length)
    d = Data(seqs, k)
    own = np.diag(d.union)
    assert set(own.tolist()) == {0, 127} and d.union.max() == 254 and (d.inter > 100).sum() > d.n
    sets = device_sets(da, seqs, k)
    assert sets.ld_keys == 128
    codes = device.jaccard_rect(sets, kind=COMPACT)
    vals = device.jaccard_rect(sets, 3, 80, 1, 77, kind=F64)
    torch.cuda.synchronize()
    assert np.array_equal(sets.counts.cpu().numpy(), own)
    assert np.array_equal(u16(codes), d.codes)
    assert same(vals.cpu().numpy(), d.J[3:80, 1:77])


def test_rect_sets_of_one_repeated_shingle(da):
    from dynaalign_amd import device
    seqs = [b"W" * 20, b"W" * 5, b"W" * 4, b"A" * 20, b"", b"WWW", b"W" * 130, b"AAAAW", b"\xff" * 9, b"\xff" * 4]
    d = Data(seqs, 4)
    assert d.J[0, 1] == d.J[0, 2] == d.J[0, 6] == 1.0 and d.J[0, 3] == 0.0 and d.J[4, 5] == 1.0 and d.J[0, 4] == 0.0 and d.J[3, 7] == 0.5
    sets = device_sets(da, seqs, 4)
    torch.cuda.synchronize()
    assert sets.counts.cpu().numpy().tolist() == [1, 1, 1, 1, 0, 0, 1, 2, 1, 1]
    assert np.array_equal(u16(device.jaccard_rect(sets, kind=COMPACT)), d.codes)
    assert same(device.jaccard_rect(sets, kind=F64).cpu().numpy(), d.J)


# ---- host entry points -----------------------------------------------------------------------------------------------------------------

def test_square_matrix(da, d4):
    got = da.similarityJaccard(d4.seqs, 4)
    assert same(got, d4.J)
    assert same(got, da.jaccard_dense(d4.seqs, 4))
    assert np.all(np.diag(got) == 1.0)
    assert same(da.similarityJaccard(d4.seqs[:70], 2), model_values(*model_counts(d4.seqs[:70], 2)))
    assert same(da.similarityJaccard(d4.seqs[-70:], 7), model_values(*model_counts(d4.seqs[-70:], 7)))


@pytest.mark.parametrize("column_major", [0, 1])
def test_cross_matrix_both_layouts(da, d4, column_major):
    from dynaalign_amd import _capi
    m = 77
    x, y = d4.seqs[:m], d4.seqs[m:]
    n = len(y)
    xr, xo = da.pack_sequences(x)
    yr, yo = da.pack_sequences(y)
    out = np.full(m * n, -7.0)
    _capi.check(_capi.load().da_similarity_jaccard_cross(xr.ctypes.data, xo.ctypes.data, m, yr.ctypes.data, yo.ctypes.data, n, 4, out.ctypes.data,
                                                         column_major))
    R = d4.J[:m, m:]
    assert same(out.reshape((n, m) if column_major else (m, n)), R.T if column_major else R)
    if not column_major:
        assert same(da.similarityJaccard_cross(x, y, 4), R)
        assert same(da.similarityJaccard_cross(y, x, 4), R.T)


def check_topk(da, d4, top, m=270):
    x, y = d4.seqs[:m], d4.seqs[m - 30:]                   # thirty strings on both sides
    R = d4.J[:m, m - 30:]
    idx, val = da.similarityJaccard_cross_topk(x, y, 4, top)
    want = np.argsort(-R, axis=1, kind="stable")[:, :top]
    assert idx.dtype == np.int32 and np.array_equal(idx, want), top
    assert same(val, np.take_along_axis(R, want, axis=1)), top


def check_knn(da, d4, top):
    idx, val = da.similarityJaccard_knn(d4.seqs, 4, top)
    widx, wval = da.knn_dense(d4.J, top)
    assert idx.dtype == np.int32 and np.array_equal(idx, widx), top
    assert same(val, wval), top


def test_cross_topk(da, d4):
    for top in (1, 10, d4.n - 240):
        check_topk(da, d4, top)


def test_knn(da, d4):
    for top in (1, 10, d4.n - 1):
        check_knn(da, d4, top)


def test_topk_and_knn_in_three_row_blocks(da, d4):
    with switches(DYNAALIGN_BLOCK_BYTES=1024):              # the smallest block, 128 rows: 270 and 310 rows are cut into three
        for top in (1, 10, d4.n - 240):
            check_topk(da, d4, top)
        for top in (1, 10, d4.n - 1):
            check_knn(da, d4, top)


def test_equal_values_of_different_codes_tie_by_position(da):
    # against "ABCD" (k = 2: AB BC CD): "ABCQRS" is 2/6 and "AB" 1/3, "ABCDEFG" is 3/6 and "ABCX" 2/4
    y = [b"ABXY", b"ABCQRS", b"AB", b"ABCDEFG", b"ABCX", b"BCD", b"CDQ"]
    x = [b"ABCD", b"ABCDEFG"]
    inter, union = model_counts(x, 2, y)
    R = model_values(inter, union)
    codes = model_codes(inter, union)
    tie = [(i, a, b) for i in range(2) for a in range(7) for b in range(a + 1, 7) if R[i, a] == R[i, b] and codes[i, a] != codes[i, b]]
    assert len(tie) >= 2, "the input holds no equal values with different codes"
    idx, val = da.similarityJaccard_cross_topk(x, y, 2, 7)
    want = np.argsort(-R, axis=1, kind="stable")
    assert np.array_equal(idx, want) and same(val, np.take_along_axis(R, want, axis=1))


@pytest.mark.parametrize("mode", ["union", "mutual"])
def test_knn_edges(da, d4, mode):
    thr, ei, ej, w = da.similarityJaccard_knn_edges(d4.seqs, 4, 10, mode)
    wi, wj, ww = da.knn_graph(*da.knn_dense(d4.J, 10), 1.0, mode)
    assert np.array_equal(ei, wi) and np.array_equal(ej, wj) and same(w, ww)
    off = ww[wi != wj]
    assert len(off) >= 100 and bits(thr) == bits(off.min())


@pytest.mark.parametrize("p", [0.0, 0.5, 0.8, 1.0])
def test_edges(da, d4, p):
    from dynaalign_amd.clusterbreak import threshold_edges_dense
    thr, ei, ej, w = da.similarityJaccard_edges(d4.seqs, 4, p)
    wthr, wi, wj, ww = threshold_edges_dense(d4.J, p)
    order, worder = np.lexsort((ej, ei)), np.lexsort((wj, wi))
    assert bits(thr) == bits(wthr), (thr, wthr)
    assert np.array_equal(ei[order], wi[worder]) and np.array_equal(ej[order], wj[worder]) and same(w[order], ww[worder])
    assert len(ei) > d4.n                                    # more than the diagonal
    if p == 0.8:
        assert thr > 0


# ---- the host entry points on 127-shingle sets: codes up to 127 << 8 | 127 = 32 639, so the threshold step's histogram has more bins than its
# LDS copy holds and the top-k rank table needs 15 bits.  Compared with the set model and numpy alone.

@pytest.fixture(scope="module", params=[(4, 130), (8, 134)], ids=["k4_u32", "k8_u64"])
def d127(request):
    k, length = request.param
    d = Data(sequences_of_127_shingles(length), k)
    up, codes = d.J[np.triu_indices(d.n, 1)], d.codes[np.triu_indices(d.n, 1)]
    # an all-zero result, or one whose codes all stay below the 8192 bins of the LDS histogram, cannot pass what follows
    assert d.n == 84 and codes.max() >= 8192 and (codes >= 8192).mean() > 0.2
    assert np.quantile(up, 0.8) > 0 and len(np.unique(up)) >= 20
    return d


def quantile_type7_of(x, p):
    """stats::quantile(x, p, type = 7) in R's arithmetic: qs = x[lo]; (1 - h) qs + h x[hi] when the index lies between two different values"""
    x = np.sort(np.asarray(x, np.float64))
    index = 1.0 + (len(x) - 1) * p
    lo, hi = int(np.floor(index)), int(np.ceil(index))
    qs, xh = float(x[lo - 1]), float(x[hi - 1])
    if index > lo and xh != qs:
        h = index - lo
        qs = (1.0 - h) * qs + h * xh
    return qs


@pytest.mark.parametrize("p", [0.0, 0.5, 0.8, 1.0])
def test_edges_of_127_shingle_sets(da, d127, p):
    thr, ei, ej, w = da.similarityJaccard_edges(d127.seqs, d127.k, p)
    wthr = quantile_type7_of(d127.J[np.triu_indices(d127.n, 1)], p)
    assert bits(thr) == bits(wthr), (thr, wthr)
    wi, wj = np.nonzero(np.triu((d127.J >= wthr) & (d127.J > 0)))              # row-major: sorted by (i, j)
    order = np.lexsort((ej, ei))
    assert np.array_equal(ei[order], wi) and np.array_equal(ej[order], wj) and same(w[order], d127.J[wi, wj])
    assert len(wi) > d127.n and (d127.codes[wi, wj] >= 8192).any()
    if p == 0.8:
        assert thr > 0
    if p == 1.0:
        assert thr == 1.0 and (wi != wj).any()                                   # the strings without a shingle among themselves


def test_knn_of_127_shingle_sets(da, d127):
    M = d127.J.copy()
    np.fill_diagonal(M, -np.inf)
    order = np.argsort(-M, axis=1, kind="stable")
    for top in (1, 10, d127.n - 1):
        idx, val = da.similarityJaccard_knn(d127.seqs, d127.k, top)
        assert idx.dtype == np.int32 and np.array_equal(idx, order[:, :top]), top
        assert same(val, np.take_along_axis(d127.J, order[:, :top], axis=1)), top


def test_cross_topk_of_127_shingle_sets(da, d127):
    m = 50
    x, y = d127.seqs[:m], d127.seqs[m:]
    assert len(y) == 34
    R = d127.J[:m, m:]
    assert len(np.unique(R)) >= 10 and (R > 0).mean() > 0.2
    order = np.argsort(-R, axis=1, kind="stable")
    for top in (1, 10, 34):
        idx, val = da.similarityJaccard_cross_topk(x, y, d127.k, top)
        assert idx.dtype == np.int32 and np.array_equal(idx, order[:, :top]), top
        assert same(val, np.take_along_axis(R, order[:, :top], axis=1)), top


def test_equal_sets_have_equal_minhash_signatures(da, d4):
    S = np.asarray(da.similarityMH(d4.seqs, 4, 50, seed=12345))
    one = d4.J == 1.0
    assert one.sum() > d4.n                                  # byte-identical strings and the strings shorter than k among themselves
    assert np.all(S[one] == 1.0)


def test_clusterbreak_on_the_edge_list_is_clusterbreak_on_the_dense_matrix(da):
    import importlib
    cb = importlib.import_module("dynaalign_amd.clusterbreak")
    pep = family(31, 12, 12, 390) + ["", "A", "AC", "W" * 12, "ACDEFGHIKLMN", "ACDEFGHIKLMN"]
    kw = dict(size_max=10, size_min=3, log=io.StringIO())
    dense = cb.clusterbreak(pep, 0.8, sim_fn=lambda s: da.jaccard_dense(s, 2), **kw)
    edges = cb.clusterbreak(pep, 0.8, edges_fn=lambda s: da.similarityJaccard_edges(s, k=2), **kw)
    assert np.array_equal(dense["clustered_seq"], edges["clustered_seq"]) and dense["filtered_seq"] == edges["filtered_seq"]
    assert dense.calls == edges.calls and dense.calls >= 3
    per_level = lambda res: [(lv["n"], np.float64(lv["threshold"]).view(np.uint64), lv["edges"]) for lv in res.levels]    # noqa: E731
    assert per_level(dense) == per_level(edges)
