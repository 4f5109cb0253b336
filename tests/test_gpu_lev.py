"""GPU tests of the Levenshtein similarity: the device layer (device.lev_masks / device.lev_rect), the host entry points (similarityLev, _cross,
_cross_topk, _knn, _knn_edges, _edges, _cross_edges) and clusterbreak on them.  The yardstick is the O(len(a) len(b)) dynamic programme,
written here cell by cell for all pairs at once -- independently of the package's lev_counts -- and every comparison is exact: indices and
codes as integers, values as uint64 bit patterns."""
import io

import numpy as np
import pytest
import torch

from test_gpu_cross import bits, same, strided, switches

pytestmark = pytest.mark.gpu

AA20 = "ACDEFGHIKLMNPQRSTVWY"
T = 64                      # tile edge of k_lev_rect
COMPACT, F64 = 1, 0
RATIO = np.array([[(num / ln) if ln else 1.0 for ln in range(128)] for num in range(128)])      # Python's divide of the two integers; 1.0 at L = 0


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    from dynaalign_amd import _capi
    assert _capi.load().da_device_count() > 0
    return dynaalign_amd


def as_bytes(seqs):
    return [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in seqs]


def dp_distance(x, y):
    """d[i, j], the Levenshtein distance of x[i] and y[j]: the textbook recurrence D[p][q] = min(D[p-1][q] + 1, D[p][q-1] + 1,
    D[p-1][q-1] + (a[p-1] != b[q-1])), one cell (p, q) at a time, for all pairs at once; pair (i, j) reads its result at (len a, len b)"""
    x, y = as_bytes(x), as_bytes(y)
    m, n = len(x), len(y)
    la, lb = np.array([len(a) for a in x]), np.array([len(b) for b in y])
    LA, LB = int(la.max()), int(lb.max())
    A = np.full((m, max(LA, 1)), -1, np.int16)
    B = np.full((n, max(LB, 1)), -2, np.int16)
    for i, a in enumerate(x):
        A[i, :len(a)] = np.frombuffer(a, np.uint8)
    for j, b in enumerate(y):
        B[j, :len(b)] = np.frombuffer(b, np.uint8)
    ii, jj = np.arange(m)[:, None], np.arange(n)[None, :]
    take = lambda row: row[lb[None, :], ii, jj]                                      # noqa: E731
    prev = np.broadcast_to(np.arange(LB + 1, dtype=np.int16)[:, None, None], (LB + 1, m, n)).copy()      # D[0][q] = q
    out = np.zeros((m, n), np.int64)
    out[la == 0] = take(prev)[la == 0]
    for p in range(1, LA + 1):
        cur = np.empty_like(prev)
        cur[0] = p
        ne = A[:, p - 1][:, None, None] != B[None, :, :]                             # (m, n, LB)
        for q in range(1, LB + 1):
            cur[q] = np.minimum(np.minimum(prev[q] + 1, cur[q - 1] + 1), prev[q - 1] + ne[:, :, q - 1])
        out[la == p] = take(cur)[la == p]
        prev = cur
    return out


def model_counts(x, y=None):
    """(L - d, L) by the DP"""
    x = as_bytes(x)
    y = x if y is None else as_bytes(y)
    longer = np.maximum(np.array([len(a) for a in x], np.int64)[:, None], np.array([len(b) for b in y], np.int64)[None, :])
    return longer - dp_distance(x, y), longer


def model_values(num, den):
    return RATIO[num, den]


def model_codes(num, den):
    return np.where(den > 0, num << 8 | den, 0x0101).astype(np.uint16)


def u16(t):
    return t.cpu().numpy().view(np.uint16)


class Data:
    def __init__(self, seqs):
        self.seqs = as_bytes(seqs)
        self.num, self.den = model_counts(self.seqs)
        self.S, self.codes = model_values(self.num, self.den), model_codes(self.num, self.den)
        self.n = len(self.seqs)
        assert np.array_equal(self.num, self.num.T) and np.all(np.diag(self.num) == np.diag(self.den))


def test_the_yardstick_on_hand_written_cases():
    d = dp_distance(["kitten", "", "ACDEFGHIKL", "ACDEFGHIKL", "ACDEFGHIKL", "A" * 127], ["sitting", "", "ACDEFGHIK", "CDEFGHIKLM", "LKIHGFEDCA", "A" * 64])
    assert np.diag(d).tolist() == [3, 0, 1, 2, 10, 63] and d[1].tolist() == [7, 0, 9, 10, 10, 64] and d[0, 1] == 6


def family(seed, parents, length, count, alphabet=AA20):
    """`count` strings: a random one of `parents` random strings over `alphabet` with 0-3 substitutions and, half the time, one residue
    dropped at the front or appended at the back (a one-residue shift: cheap for the edit distance, fatal for a position-wise compare)"""
    rng = np.random.RandomState(seed)
    par = ["".join(alphabet[t] for t in rng.randint(0, len(alphabet), length)) for _ in range(parents)]
    out = []
    for _ in range(count):
        s = list(par[rng.randint(0, parents)])
        for _ in range(rng.randint(0, 4)):
            s[rng.randint(0, len(s))] = alphabet[rng.randint(0, len(alphabet))]
        s = "".join(s)
        if rng.randint(0, 2):
            s = s[1:] if rng.randint(0, 2) else s + alphabet[rng.randint(0, len(alphabet))]
        out.append(s)
    return out


def edge_strings():
    return [b"", b"", b"A", b"AC", b"W" * 20, b"ACDEFGHIKLMNPQRSTV\x80", b"ACDEFGHIKLMNPQR\xe9\xff", b"AC\xff\x00\xff\xffDEFGHIKLMN",
            b"ACDEFGHIKLMNPQRSTVWY", b"ACDEFGHIKLMNPQRSTVWY"]


def shape_set(cap, alphabet, seed):
    """strings of every length at which a word shape can go wrong, up to `cap` bytes: 0, 1, B - 1, B, B + 1 for B = 32 and 64 where they fit,
    cap - 1 and cap.  Per length a random string over `alphabet` (a sequence of byte values), a copy with one substitution, and the copy
    shifted by one residue (cut to the cap): near-copies, whose distances are small and differ at the last pattern bit -- bit 31 or 63
    of word 0, bit 0 (length 65) or 62 (length 127) of word 1.  Then the carry cases: all-equal strings of 64, 65 and `cap` bytes, and
    copies of one string that differ only at position 63 or 64."""
    rng = np.random.RandomState(seed)
    draw = lambda k: bytes(alphabet[t] for t in rng.randint(0, len(alphabet), k))     # noqa: E731
    out = []
    for ln in sorted({0, 1, 2, 31, 32, 33, 63, 64, 65, cap - 1, cap}):
        if ln > cap:
            continue
        s = draw(ln)
        out.append(s)
        if ln:
            t = bytearray(s)
            t[rng.randint(0, ln)] = alphabet[rng.randint(0, len(alphabet))]
            out.append(bytes(t))
            out.append((draw(1) + bytes(t))[:cap])
    a = bytes([alphabet[0]])
    out += [a * cap, a * min(cap, 64), a * min(cap, 65), a * cap, a * (cap - 1)]
    base = bytearray(draw(cap))
    for pos in (31, 32, 63, 64):
        if pos < cap:
            t = bytearray(base)
            t[pos] = alphabet[1] if t[pos] != alphabet[1] else alphabet[0]
            out.append(bytes(t))
    out.append(bytes(base))
    return out


def device_masks(da, seqs, class_map=None):
    from dynaalign_amd import device
    res, off = da.pack_sequences(seqs)
    return device.lev_masks(device.DeviceSequences(res, off), class_map)


ALPHABETS = {
    "two": list(b"AB"),
    "aa20": list(AA20.encode()),
    "forty": [0x00, 0x80, 0xFF] + list(range(60, 97)),       # more than 32 distinct byte values, 0x00 / 0x80 / 0xFF among them
    "all256": list(range(256)),
}


# ---- device layer ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("alphabet", list(ALPHABETS))
@pytest.mark.parametrize("cap", [32, 64, 127])
def test_rect_every_word_shape_and_alphabet(da, cap, alphabet):
    """the three template instances (one uint32, one uint64, two uint64) on their own edge lengths and carry cases, under 2, 20, 40 and 256
    classes: with 256 the match masks of a tile's 64 rows no longer fit the LDS budget and are staged in several rounds"""
    from dynaalign_amd import device
    letters = ALPHABETS[alphabet]
    seqs = shape_set(cap, letters, cap + len(letters))
    if alphabet == "all256":                                     # every byte value occurs: 256 classes
        seqs += [bytes(range(c, min(c + cap, 256))) for c in range(0, 256, cap)]
        seqs += family(cap, 2, cap - 1, 50, [chr(c) for c in letters])                        # ... and more than one tile of rows
    d = Data(seqs)
    assert max(len(s) for s in d.seqs) == cap and len(np.unique(d.codes)) >= 12
    masks = device_masks(da, d.seqs)
    assert masks.n_classes == len(set(b"".join(d.seqs))) and (alphabet != "all256" or (masks.n_classes == 256 and d.n > T))
    codes = device.lev_rect(masks, kind=COMPACT)
    vals = device.lev_rect(masks, kind=F64)
    torch.cuda.synchronize()
    assert np.array_equal(u16(codes), d.codes)
    assert same(vals.cpu().numpy(), d.S)
    assert (d.codes & 0xFF).min() >= 1 and not np.isnan(d.S).any()


def test_rect_carries_across_the_word_boundary(da):
    """the cases of the two-word recurrence by name: equal letters all along (the addition's carry runs through bit 63 into word 1), and copies
    that differ only at position 63 or 64 (both shifts carry a bit from word 0 into word 1)"""
    from dynaalign_amd import device
    rng = np.random.RandomState(4)
    base = bytes(rng.randint(65, 69, 127).astype(np.uint8))
    flip = lambda pos: base[:pos] + bytes([base[pos] ^ 0x20]) + base[pos + 1:]       # noqa: E731
    seqs = [b"A" * 127, b"A" * 64, b"A" * 65, b"A" * 127, b"A" * 63, b"B" + b"A" * 126, b"A" * 126 + b"B", base, flip(63), flip(64), flip(62), flip(126),
            base[1:], base[:64], base[:65], base[64:], b""]
    d = Data(seqs)
    dist = d.den - d.num
    assert dist[0, 1:5].tolist() == [63, 62, 0, 64] and dist[7, 8:13].tolist() == [1, 1, 1, 1, 1] and dist[8, 9] == 2
    masks = device_masks(da, seqs)
    codes = device.lev_rect(masks, kind=COMPACT)
    vals = device.lev_rect(masks, kind=F64)
    torch.cuda.synchronize()
    assert np.array_equal(u16(codes), d.codes) and same(vals.cpu().numpy(), d.S)


def test_rect_all_strings_empty_and_a_callers_class_map(da):
    from dynaalign_amd import device
    masks = device_masks(da, [b"", b"", b""])
    assert masks.n_classes == 1 and masks.max_len == 0
    codes = device.lev_rect(masks, kind=COMPACT)
    vals = device.lev_rect(masks, kind=F64)
    torch.cuda.synchronize()
    assert np.all(u16(codes) == 0x0101) and np.all(vals.cpu().numpy() == 1.0)
    # the caller's own map: the identity over 256 classes, and one that folds the bytes that do not occur onto class 0
    d = Data(family(9, 3, 20, 40) + edge_strings())
    used = sorted(set(b"".join(d.seqs)))
    fold = np.zeros(256, np.uint8)
    fold[used] = np.arange(len(used))[::-1]                      # any numbering of the bytes that occur will do
    for class_map in (np.arange(256, dtype=np.uint8), fold):
        masks = device_masks(da, d.seqs, class_map)
        assert masks.n_classes == int(class_map.max()) + 1
        codes = device.lev_rect(masks, kind=COMPACT)
        torch.cuda.synchronize()
        assert np.array_equal(u16(codes), d.codes)


@pytest.fixture(scope="module")
def d20():
    """290 near-copy 20-mers of 3 families (substitutions and one-residue shifts) + the edge strings: the input of the host-boundary tests, its
    model computed once"""
    d = Data(family(11, 3, 20, 290) + edge_strings())
    up = d.S[np.triu_indices(d.n, 1)]
    # a wrong all-zero result cannot pass what follows
    assert (up > 0).mean() >= 0.85 and len(np.unique(up)) >= 25 and np.quantile(up, 0.8) > 0.5
    return d


@pytest.mark.parametrize("n", [1, 2, T - 1, T, T + 1, 2 * T + 2])
def test_rect_full_square_at_the_tile_edges(da, d20, n):
    from dynaalign_amd import device
    lo = d20.n - n                                               # the edge strings are among them
    masks = device_masks(da, d20.seqs[lo:])
    codes = device.lev_rect(masks, kind=COMPACT)
    vals = device.lev_rect(masks, kind=F64)
    torch.cuda.synchronize()
    assert np.array_equal(u16(codes), d20.codes[lo:, lo:])
    assert same(vals.cpu().numpy(), d20.S[lo:, lo:])


RECTS = [(0, 1, 0, 1), (5, 70, 3, 131), (63, 66, 0, 200), (0, 200, 64, 65), (1, 130, 1, 130), (100, 197, 37, 180), (37, 180, 100, 197),
         (128, 200, 0, 128), (7, 7, 0, 200), (0, 200, 9, 9)]


@pytest.mark.parametrize("kind", [COMPACT, F64], ids=["codes", "f64"])
def test_rect_odd_rectangles_odd_ld_and_offset_base(da, d20, kind):
    """origins and extents that are no tile multiples, row and column ranges that overlap the diagonal (one of them the symmetric form), an
    odd leading dimension and a base one element into its allocation; what lies around the rectangle stays as it was"""
    from dynaalign_amd import _capi, device
    n = 200
    lo = d20.n - n
    masks = device_masks(da, d20.seqs[lo:])
    want_all = d20.codes if kind == COMPACT else d20.S
    dtype = torch.int16 if kind == COMPACT else torch.float64
    for r0, r1, c0, c1 in RECTS:
        rows, cols = r1 - r0, c1 - c0
        for ld, offset in ((cols, 0), (cols + 1 + cols % 2, 1), (cols + 8, 3)):      # the second: odd, whatever cols is
            buf, view = strided(max(rows, 1), max(cols, 1), max(ld, 1), dtype, offset)
            if rows and cols:
                device.lev_rect(masks, r0, r1, c0, c1, kind=kind, out=view)
            else:                                            # an empty rectangle is DA_OK and touches nothing
                _capi.check(_capi.load().da_dev_lev_rect(masks.masks.data_ptr(), n, masks.max_len, masks.n_classes, r0, r1, c0, c1, kind,
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


@pytest.mark.parametrize("kind", [COMPACT, F64], ids=["codes", "f64"])
def test_symmetric_launch_equals_the_plain_rectangles(da, d20, kind):
    """a square range of more than one tile launches only the tiles on and above the diagonal and mirrors them; the same elements computed as
    rows x all columns (no square range: every tile launched) must be identical, tile multiples or not"""
    from dynaalign_amd import device
    n = 200
    masks = device_masks(da, d20.seqs[:n])
    for r0, r1 in ((0, 200), (5, 198), (64, 192), (3, 68)):
        sym = device.lev_rect(masks, r0, r1, r0, r1, kind=kind)
        plain = device.lev_rect(masks, r0, r1, 0, n, kind=kind)[:, r0:r1]
        torch.cuda.synchronize()
        assert torch.equal(sym, plain), (r0, r1)
        want = d20.codes[r0:r1, r0:r1] if kind == COMPACT else d20.S[r0:r1, r0:r1]
        assert np.array_equal(u16(sym), want) if kind == COMPACT else same(sym.cpu().numpy(), want)


# ---- host entry points -----------------------------------------------------------------------------------------------------------------

def test_square_matrix(da, d20):
    got = da.similarityLev(d20.seqs)
    assert same(got, d20.S)
    sub = d20.seqs[:40] + d20.seqs[-10:]
    assert same(da.similarityLev(sub), da.lev_dense(sub))
    assert np.all(np.diag(got) == 1.0) and np.array_equal(np.asarray(got), np.asarray(got).T)
    assert same(da.similarityLev(["", ""]), np.ones((2, 2))) and same(da.similarityLev(["", "A"]), np.eye(2))
    assert same(da.similarityLev(["kitten", "sitting"]), np.array([[1.0, 4 / 7], [4 / 7, 1.0]]))
    assert same(da.similarityLev(["kitten", b"kitten"]), np.ones((2, 2)))                      # str and bytes alike


@pytest.mark.parametrize("column_major", [0, 1])
def test_cross_matrix_both_layouts(da, d20, column_major):
    from dynaalign_amd import _capi
    m = 77
    x, y = d20.seqs[:m], d20.seqs[m:]
    n = len(y)
    xr, xo = da.pack_sequences(x)
    yr, yo = da.pack_sequences(y)
    out = np.full(m * n, -7.0)
    _capi.check(_capi.load().da_similarity_lev_cross(xr.ctypes.data, xo.ctypes.data, m, yr.ctypes.data, yo.ctypes.data, n, out.ctypes.data, column_major))
    R = d20.S[:m, m:]
    assert same(out.reshape((n, m) if column_major else (m, n)), R.T if column_major else R)
    if not column_major:
        assert same(da.similarityLev_cross(x, y), R)
        assert same(da.similarityLev_cross(y, x), R.T)


def check_topk(da, d, top, m):
    x, y = d.seqs[:m], d.seqs[m - 30:]                     # thirty strings on both sides
    R = d.S[:m, m - 30:]
    idx, val = da.similarityLev_cross_topk(x, y, top)
    want = np.argsort(-R, axis=1, kind="stable")[:, :top]
    assert idx.dtype == np.int32 and np.array_equal(idx, want), top
    assert same(val, np.take_along_axis(R, want, axis=1)), top


def check_knn(da, d, top):
    idx, val = da.similarityLev_knn(d.seqs, top)
    widx, wval = da.knn_dense(d.S, top)
    assert idx.dtype == np.int32 and np.array_equal(idx, widx), top
    assert same(val, wval), top


def test_cross_topk(da, d20):
    for top in (1, 10, d20.n - 240):
        check_topk(da, d20, top, 270)


def test_knn(da, d20):
    for top in (1, 10, d20.n - 1):
        check_knn(da, d20, top)


@pytest.fixture(scope="module")
def two_letter():
    """150 strings of 6 .. 12 letters over A and B: few distinct values, and equal values of different codes (4/8, 5/10, 6/12) in every row"""
    rng = np.random.RandomState(17)
    d = Data(["".join("AB"[t] for t in rng.randint(0, 2, rng.randint(6, 13))) for _ in range(150)])
    ties = sum(len(np.unique(d.codes[i])) - len(np.unique(d.S[i])) for i in range(d.n))
    assert len(np.unique(d.S)) <= 60 and ties >= 2 * d.n
    return d


def test_equal_values_of_different_codes_tie_by_position(da, two_letter):
    for top in (1, 7, 60):
        check_topk(da, two_letter, top, 100)
    for top in (1, 7, two_letter.n - 1):
        check_knn(da, two_letter, top)


def cross_edges_of(R, thr):
    wi, wj = np.nonzero((R >= thr) & (R > 0))              # row-major: sorted by (i, j)
    return wi, wj, R[wi, wj]


def check_cross_edges(da, d, m):
    x, y = d.seqs[:m], d.seqs[m:]
    R = d.S[:m, m:]
    for threshold in (0.8, 0.5, 1.0, 0.0, 1.5):
        thr, ei, ej, w = da.similarityLev_cross_edges(x, y, threshold=threshold)
        wi, wj, ww = cross_edges_of(R, threshold)
        assert bits(thr) == bits(threshold) and np.array_equal(ei, wi) and np.array_equal(ej, wj) and same(w, ww), threshold
    thr, ei, ej, w = da.similarityLev_cross_edges(x, y, 0.8)
    wthr = quantile_type7_of(R.ravel(), 0.8)
    wi, wj, ww = cross_edges_of(R, wthr)
    assert bits(thr) == bits(wthr) and np.array_equal(ei, wi) and np.array_equal(ej, wj) and same(w, ww) and len(wi) > 100


def test_topk_knn_and_cross_edges_in_three_row_blocks(da, d20):
    with switches(DYNAALIGN_BLOCK_BYTES=1024):              # the smallest block, 128 rows: 270 and 300 rows are cut into three
        for top in (1, 10, d20.n - 240):
            check_topk(da, d20, top, 270)
        for top in (1, 10, d20.n - 1):
            check_knn(da, d20, top)
        check_cross_edges(da, d20, 270)


@pytest.mark.parametrize("mode", ["union", "mutual"])
def test_knn_edges(da, d20, mode):
    thr, ei, ej, w = da.similarityLev_knn_edges(d20.seqs, 10, mode)
    wi, wj, ww = da.knn_graph(*da.knn_dense(d20.S, 10), 1.0, mode)
    assert np.array_equal(ei, wi) and np.array_equal(ej, wj) and same(w, ww)
    off = ww[wi != wj]
    assert len(off) >= 100 and bits(thr) == bits(off.min())


@pytest.mark.parametrize("p", [0.0, 0.8, 1.0])
def test_edges(da, d20, p):
    from dynaalign_amd.clusterbreak import threshold_edges_dense
    thr, ei, ej, w = da.similarityLev_edges(d20.seqs, p)
    wthr, wi, wj, ww = threshold_edges_dense(d20.S, p)
    order, worder = np.lexsort((ej, ei)), np.lexsort((wj, wi))
    assert bits(thr) == bits(wthr), (thr, wthr)
    assert np.array_equal(ei[order], wi[worder]) and np.array_equal(ej[order], wj[worder]) and same(w[order], ww[worder])
    assert len(ei) > d20.n                                   # more than the diagonal
    if p == 0.8:
        assert thr > 0


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


def test_cross_edges(da, d20):
    check_cross_edges(da, d20, 120)


def test_cross_edges_within_one_and_two_edits(da, d20):
    """with all strings of length L, "within t edits" is the threshold (L - t) / L: the positions are those of the DP's distance"""
    L = 20
    full = [s for s in d20.seqs if len(s) == L]
    assert len(full) >= 120
    x, y = full[:50], full[50:]
    dist = dp_distance(x, y)
    assert (dist == 1).sum() >= 20 and (dist == 2).sum() >= 20 and (dist == 0).sum() >= 1 and (dist > 2).sum() >= 20
    for t in (1, 2):
        thr, ei, ej, w = da.similarityLev_cross_edges(x, y, threshold=(L - t) / L)
        wi, wj = np.nonzero(dist <= t)
        assert bits(thr) == bits((L - t) / L) and np.array_equal(ei, wi) and np.array_equal(ej, wj), t
        assert same(w, RATIO[L - dist[wi, wj], L]), t


def test_cross_edges_of_127_byte_strings(da):
    """codes up to 127 << 8 | 127 = 32 639: the threshold step's histogram has more bins than its LDS copy holds"""
    d = Data(family(6, 2, 126, 60) + shape_set(127, ALPHABETS["aa20"], 5)[:20])
    m = 30
    R = d.S[:m, m:]
    assert d.codes[:m, m:].max() >= 8192 and (d.codes[:m, m:] >= 8192).mean() > 0.2
    check_cross_edges(da, d, m)


def test_clusterbreak_on_the_edge_list_is_clusterbreak_on_the_dp_matrix(da):
    import importlib
    cb = importlib.import_module("dynaalign_amd.clusterbreak")
    pep = family(31, 12, 12, 390) + ["", "A", "AC", "W" * 12, "ACDEFGHIKLMN", "ACDEFGHIKLMN"]
    kw = dict(size_max=10, size_min=3, log=io.StringIO())
    dense = cb.clusterbreak(pep, 0.8, sim_fn=lambda s: model_values(*model_counts(list(s))), **kw)
    edges = cb.clusterbreak(pep, 0.8, edges_fn=lambda s: da.similarityLev_edges(s), **kw)
    assert np.array_equal(dense["clustered_seq"], edges["clustered_seq"]) and dense["filtered_seq"] == edges["filtered_seq"]
    assert dense.calls == edges.calls and dense.calls >= 3
    per_level = lambda res: [(lv["n"], np.float64(lv["threshold"]).view(np.uint64), lv["edges"]) for lv in res.levels]    # noqa: E731
    assert per_level(dense) == per_level(edges)
