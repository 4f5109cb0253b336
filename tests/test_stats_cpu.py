"""CPU tests of the similarity statistics: compute_similarity_stats (the reference's R/similarity.R:11-34 in numpy) on hand-written matrices,
da_stats_from_histogram against numpy on expanded multisets, and the C boundary of da_similarity_mh_stats / da_similarity_nw_stats /
da_similarity_nw_stats_long and of the two device entries -- symbols, signatures, every refusal with its text before DA_ERR_NO_DEVICE.
No compute calls here.  Doubles are compared as uint64 bit patterns; the mean against math.fsum(U) / P within 2 ** -40 relative: each of
the <= 2 ** 21 products and adds of the long double sum errs by at most 2 ** -64 relative and every term is >= 0, which bounds the result
within 2 ** -42 of the exact mean of the doubles; one spare factor of 4 for the reference's own two roundings."""
import ctypes
import math
import warnings
from fractions import Fraction

import numpy as np
import pytest

import oracle_lib as O

OK, EMPTY_INPUT, BAD_K, BAD_NHASH, BAD_MATRIX, NO_DEVICE, UNSUPPORTED, BAD_ARG = 0, 1, 2, 3, 4, 8, 10, 11
MEAN_RTOL = 2.0 ** -40
SYMBOLS = ["da_stats_from_histogram", "da_similarity_mh_stats", "da_similarity_nw_stats", "da_similarity_nw_stats_long", "da_dev_upper_extrema",
           "da_dev_upper_extrema32"]


@pytest.fixture(scope="module")
def lib(built):
    from dynaalign_amd import _capi
    return _capi.load()


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    return dynaalign_amd


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def expected(R):
    """the issue's recipe on a dense matrix: (mean by fsum, median, min, max, pair, pair, upper, upper)"""
    n = R.shape[0]
    U = R[np.triu_indices(n, 1)]

    def pair(v):
        return tuple(int(t) for t in np.argwhere(R.T == v)[0][::-1])

    def upper(v):
        return tuple(int(t) for t in np.argwhere(np.triu(R == v, 1))[0])
    return (math.fsum(U) / U.size, float(np.median(U)), float(U.min()), float(U.max()), pair(U.max()), pair(U.min()), upper(U.max()), upper(U.min()))


def assert_stats(got, R, what=""):
    want = expected(R)
    assert abs(got.mean_similarity - want[0]) <= MEAN_RTOL * abs(want[0]), (what, got.mean_similarity, want[0])
    for name, w in zip(("median_similarity", "min_similarity", "max_similarity"), want[1:4]):
        assert bits(getattr(got, name)) == bits(w), (what, name, getattr(got, name), w)
    for name, w in zip(("most_similar_pair", "least_similar_pair", "most_similar_upper", "least_similar_upper"), want[4:]):
        assert tuple(getattr(got, name)) == w, (what, name, getattr(got, name), w)


def sym(upper_rows, diag=1.0):
    """symmetric matrix from the rows of its strict upper triangle"""
    n = len(upper_rows) + 1
    R = np.full((n, n), diag, np.float64)
    for i, row in enumerate(upper_rows):
        assert len(row) == n - 1 - i
        for t, v in enumerate(row):
            R[i, i + 1 + t] = R[i + 1 + t, i] = v
    return R


# ---- compute_similarity_stats -----------------------------------------------------------------------------------------------------------------

def test_exports_and_fields(da):
    for name in ("SimilarityStats", "compute_similarity_stats", "stats_from_histogram", "similarityMH_stats", "similarityNW_stats",
                 "similarityNW_stats_long"):
        assert name in da.__all__ and hasattr(da, name), name
    assert da.SimilarityStats._fields == ("mean_similarity", "median_similarity", "min_similarity", "max_similarity", "most_similar_pair",
                                          "least_similar_pair", "most_similar_upper", "least_similar_upper")
    import inspect
    from dynaalign_amd import device
    from dynaalign_amd.session import MinHashSession
    assert list(inspect.signature(device.upper_extrema).parameters) == ["keys", "n", "rank", "row_begin", "col_begin"]
    assert list(inspect.signature(MinHashSession.stats).parameters) == ["self", "idx"]
    assert inspect.signature(da.similarityNW_stats) == inspect.signature(da.similarityNW_stats_long)


def test_two_by_two(da):
    R = sym([[0.25]])
    s = da.compute_similarity_stats(R)
    assert (s.mean_similarity, s.median_similarity, s.min_similarity, s.max_similarity) == (0.25, 0.25, 0.25, 0.25)
    assert s.most_similar_pair == s.least_similar_pair == (1, 0)          # column-major over the whole matrix: the lower triangle's copy comes first
    assert s.most_similar_upper == s.least_similar_upper == (0, 1)
    assert_stats(s, R)
    assert s == tuple(s) and s._asdict()["max_similarity"] == 0.25 and s[3] == 0.25


def test_column_major_and_row_major_disagree_about_first(da):
    # the maximum 0.9 at (0, 3) and (1, 2): row-major meets (0, 3) first, column-major (over the upper triangle) (1, 2); over the whole matrix
    # R's rule finds the mirrored copies first -- column 0 holds (3, 0)
    R = sym([[0.1, 0.2, 0.9], [0.9, 0.3], [0.1]])
    s = da.compute_similarity_stats(R)
    assert s.most_similar_upper == (0, 3) and s.most_similar_pair == (3, 0)
    assert s.least_similar_upper == (0, 1) and s.least_similar_pair == (1, 0)
    assert_stats(s, R)
    # the same values placed so that the first row holding the maximum is not row 0
    R = sym([[0.1, 0.2, 0.3], [0.2, 0.9], [0.9]])
    s = da.compute_similarity_stats(R)
    assert s.most_similar_upper == (1, 3) and s.most_similar_pair == (3, 1)
    assert_stats(s, R)


def test_a_maximum_equal_to_the_diagonal_lands_on_it(da):
    R = sym([[0.5, 0.25, 0.5], [0.75, 1.0], [0.5]])                         # (1, 3) are duplicates: 1.0 off the diagonal
    s = da.compute_similarity_stats(R)
    assert s.max_similarity == 1.0 and s.most_similar_pair == (0, 0) and s.most_similar_upper == (1, 3)
    assert_stats(s, R)
    # a diagonal that is not 1.0 (NW with free gaps): the minimum equals it, the maximum does not
    R = sym([[0.5, 0.25], [0.75]], diag=0.25)
    s = da.compute_similarity_stats(R)
    assert s.least_similar_pair == (0, 0) and s.least_similar_upper == (0, 2) and s.most_similar_pair == (2, 1)
    assert_stats(s, R)


def test_median_for_even_and_odd_pair_counts(da):
    R3 = sym([[0.1, 0.7], [0.2]])                                          # P = 3
    assert da.compute_similarity_stats(R3).median_similarity == 0.2
    R4 = sym([[0.1, 0.7, 0.3], [0.2, 0.6], [0.9]])                         # P = 6: (0.3 + 0.6) / 2
    assert bits(da.compute_similarity_stats(R4).median_similarity) == bits((0.3 + 0.6) / 2)
    # three of each: the two middle elements are lo and hi, and the median is their plain average
    lo, hi = 0.1, 0.3
    R = sym([[lo, hi, lo], [hi, lo], [hi]])
    assert bits(da.compute_similarity_stats(R).median_similarity) == bits(np.median([lo, hi, lo, hi, lo, hi]))
    for M in (R3, R4, R):
        assert_stats(da.compute_similarity_stats(M), M)


def test_random_matrices_against_numpy(da):
    rng = np.random.RandomState(5)
    for n in (2, 3, 7, 30):
        vals = rng.randint(0, 6, (n, n)) / 5.0                              # few values: ties everywhere
        R = np.triu(vals, 1) + np.triu(vals, 1).T + np.eye(n)
        assert_stats(da.compute_similarity_stats(da.SimilarityMatrix(R)), R, n)


def test_the_two_input_checks(da):
    for bad in ([[1.0, 0.5], [0.5, 1.0]], np.zeros(4), np.zeros((2, 2, 2)), None, 3.0):
        with pytest.raises(ValueError, match="Input must be a matrix"):
            da.compute_similarity_stats(bad)
    R = sym([[0.1, 0.7], [0.2]])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        da.compute_similarity_stats(R)                                     # symmetric: silent
    R[2, 0] = 0.5
    with pytest.warns(UserWarning, match="Input matrix is not symmetric. Results may be unexpected."):
        s = da.compute_similarity_stats(R)
    assert s.max_similarity == 0.7                                         # the upper triangle is what counts
    with pytest.raises(ValueError):
        da.compute_similarity_stats(np.ones((1, 1)))


# ---- da_stats_from_histogram ---------------------------------------------------------------------------------------------------------------------

def raw_hist(lib, hist, values, nbins=None, want=(1, 1, 1, 1)):
    h = np.ascontiguousarray(hist, np.uint64)
    v = np.ascontiguousarray(values, np.float64)
    out = np.full(4, -7.0)
    ptrs = [out[i:].ctypes.data if w else None for i, w in enumerate(want)]
    rc = lib.da_stats_from_histogram(h.ctypes.data, v.ctypes.data, len(h) if nbins is None else nbins, *ptrs)
    return rc, out


@pytest.mark.parametrize("hist,values", [
    ([1], [0.3]),                                                          # P = 1
    ([0, 2, 0], [0.0, 0.3, 1.0]),                                          # P = 2, one occupied bin
    ([1, 0, 1], [0.1, 0.2, 0.7]),                                          # P = 2, the two middle elements in different bins
    ([1, 1, 1], [0.1, 0.3, 0.7]),                                          # P = 3
    ([2, 1], [0.1, 0.3]),                                                  # P = 3, the middle inside a bin
    ([3, 0, 3], [0.1, 0.2, 0.3]),                                          # even, middle elements in different bins: (0.1 + 0.3) / 2
    ([5, 4, 0, 1], [0.0, 0.02, 0.5, 1.0]),                                 # even, both middle elements in the first bin
    ([0, 0, 7], [0.0, 0.5, 1.0]),
    (list(range(1, 52)), [c / 50 for c in range(51)]),                      # MinHash-shaped
])
def test_histogram_statistics_against_numpy_on_the_expanded_multiset(lib, da, hist, values):
    U = np.repeat(np.asarray(values, np.float64), hist)
    rc, out = raw_hist(lib, hist, values)
    assert rc == OK
    assert abs(out[0] - math.fsum(U) / U.size) <= MEAN_RTOL * (math.fsum(U) / U.size)
    assert bits(out[1]) == bits(np.median(U)) and bits(out[2]) == bits(U.min()) and bits(out[3]) == bits(U.max())
    assert da.stats_from_histogram(hist, values) == tuple(out)


def test_histogram_counts_above_2_to_the_32(lib):
    values = np.array([0.0, 0.1, 0.3, 0.7, 1.0])
    for hist in ([1 << 33, 0, (1 << 33) + 1, 0, 0],                       # odd total: the middle is the first element of bin 2
                 [1 << 33, 0, 1 << 33, 0, 0],                             # even: the middle straddles bins 0 and 2
                 [(1 << 40) + 3, 5, (1 << 34), 7, (1 << 40) + 1],
                 [3, 1 << 62, 5, 0, 0]):
        rc, out = raw_hist(lib, hist, values)
        assert rc == OK
        total = sum(hist)
        cum = np.cumsum([int(h) for h in hist], dtype=object)

        def at(pos):
            return values[next(b for b in range(len(hist)) if pos < cum[b])]
        want_median = at((total - 1) // 2) if total % 2 else (at(total // 2 - 1) + at(total // 2)) / 2.0
        exact = sum(Fraction(int(h)) * Fraction(float(v)) for h, v in zip(hist, values)) / total
        assert bits(out[1]) == bits(want_median), hist
        assert abs(Fraction(float(out[0])) - exact) <= Fraction(MEAN_RTOL) * exact, hist
        occupied = [v for h, v in zip(hist, values) if h]
        assert out[2] == occupied[0] and out[3] == occupied[-1]


def test_histogram_arguments(lib):
    assert raw_hist(lib, [0, 0], [0.1, 0.2])[0] == BAD_ARG and lib.da_last_error() == b"statistics of an empty set"
    assert raw_hist(lib, [1], [0.1], nbins=0)[0] == BAD_ARG and raw_hist(lib, [1], [0.1], nbins=-1)[0] == BAD_ARG
    v = np.array([0.5])
    assert lib.da_stats_from_histogram(None, v.ctypes.data, 1, None, None, None, None) == BAD_ARG
    assert lib.da_stats_from_histogram(v.ctypes.data, None, 1, None, None, None, None) == BAD_ARG
    rc, out = raw_hist(lib, [2, 1], [0.1, 0.3], want=(0, 1, 0, 0))            # any output may be NULL
    assert rc == OK and out[1] == 0.1 and out[0] == out[2] == out[3] == -7.0


# ---- the C boundary ------------------------------------------------------------------------------------------------------------------------------

def test_header_library_and_signatures_agree(lib):
    from dynaalign_amd import _capi
    declared = _capi.header_symbols()
    for name in SYMBOLS:
        assert name in declared and name in _capi.SIGNATURES and hasattr(lib, name), name
    assert sorted(_capi.SIGNATURES) == declared
    assert ctypes.sizeof(_capi.DaSimilarityStats) == 4 * 8 + 8 + 4 * 16


def raw_mh(lib, seqs, k=4, n_hash=50, residues=True, seeds=True, out=True):
    res, off = O.pack(seqs)
    sv = np.arange(max(n_hash, 1), dtype=np.uint32)
    from dynaalign_amd import _capi
    s = _capi.DaSimilarityStats()
    rc = lib.da_similarity_mh_stats(res.ctypes.data if residues else None, off.ctypes.data, len(seqs), k, n_hash, sv.ctypes.data if seeds else None,
                                    ctypes.addressof(s) if out else None)
    return rc, (lib.da_last_error().decode("latin-1") if rc else "")


def raw_nw(lib, seqs, matrix=b"BLOSUM62", entry="da_similarity_nw_stats", residues=True, out=True):
    res, off = O.pack(seqs)
    from dynaalign_amd import _capi
    s = _capi.DaSimilarityStats()
    rc = getattr(lib, entry)(res.ctypes.data if residues else None, off.ctypes.data, len(seqs), matrix, 10, 4, ctypes.addressof(s) if out else None)
    return rc, (lib.da_last_error().decode("latin-1") if rc else "")


def reaches_the_device(lib, rc, msg):
    """valid input: DA_OK where there is a device, DA_ERR_NO_DEVICE -- the last check -- where there is none"""
    if lib.da_device_count() > 0:
        return rc == OK
    return rc == NO_DEVICE and "no CPU fallback" in msg


def test_mh_validation_order_and_texts(lib, kats, da):
    two = ["ACDEFGHIKL", "ACDEFGHIKM"]
    # the reference's three checks first, in its order, whatever else is wrong
    assert raw_mh(lib, [], k=0, n_hash=0)[0] == EMPTY_INPUT
    assert raw_mh(lib, ["AAAA"], k=0, n_hash=0)[0] == BAD_K
    assert raw_mh(lib, ["AAAA"], n_hash=0)[0] == BAD_NHASH
    assert raw_mh(lib, [], residues=False)[0] == EMPTY_INPUT
    # NULL pointers before n < 2, n < 2 before n_hash > 65535
    for kw in ({"residues": False}, {"seeds": False}, {"out": False}):
        assert raw_mh(lib, two, **kw) == (BAD_ARG, "NULL pointer")
        assert raw_mh(lib, two[:1], n_hash=70000, **kw) == (BAD_ARG, "NULL pointer")
    rc, msg = raw_mh(lib, two[:1])
    assert rc == BAD_ARG and "need >= 2 sequences" in msg
    assert raw_mh(lib, two[:1], n_hash=70000) == (rc, msg)
    rc, msg = raw_mh(lib, two, n_hash=65536)
    assert rc == UNSUPPORTED and "n_hash <= 65535 (got 65536)" in msg
    rc2, msg2 = raw_mh(lib, two, n_hash=65536)
    assert (rc2, msg2) == (rc, msg)
    # the same refusal, the same text as the edge form's
    res, off = O.pack(two)
    sv = np.zeros(65536, np.uint32)
    thr, cnt = ctypes.c_double(), ctypes.c_int64()
    assert lib.da_similarity_mh_edges(res.ctypes.data, off.ctypes.data, 2, 4, 65536, sv.ctypes.data, 0.8, ctypes.addressof(thr), ctypes.addressof(cnt),
                                      0, None, None, None) == UNSUPPORTED
    assert lib.da_last_error().decode() == msg
    assert reaches_the_device(lib, *raw_mh(lib, two))
    assert reaches_the_device(lib, *raw_mh(lib, two, n_hash=500))
    with pytest.raises(da.DynaAlignError) as ei:
        da.similarityMH_stats(two[:1], seed=1)
    assert ei.value.code == BAD_ARG and "need >= 2 sequences" in str(ei.value)
    with pytest.raises(da.DynaAlignError) as ei:
        da.similarityMH_stats([], seed=1)
    assert (ei.value.code, str(ei.value)) == (EMPTY_INPUT, "Input sequences vector cannot be empty")


@pytest.mark.parametrize("entry,limit", [("da_similarity_nw_stats", 127), ("da_similarity_nw_stats_long", 1024)])
def test_nw_validation_order_and_texts(lib, kats, da, entry, limit):
    too_long = "ACDEFGHIKL" * 103                                                  # 1030 residues
    over = "A" * (limit + 1)
    # the matrix first, whatever else is wrong
    for seqs in (["AA", "AC"], ["AA"], [], ["AJ", "AA"], ["", "AA"], [too_long, "AA"]):
        assert raw_nw(lib, seqs, b"PAM250", entry) == (BAD_MATRIX, kats["nw_bad_matrix"]["error"]), seqs[:1]
    assert raw_nw(lib, ["AA"], b"PAM250", entry, residues=False)[0] == BAD_MATRIX
    # NULL pointers before n < 2
    for kw in ({"residues": False}, {"out": False}):
        assert raw_nw(lib, ["AA", "AC"], entry=entry, **kw) == (BAD_ARG, "NULL pointer")
        assert raw_nw(lib, ["AA"], entry=entry, **kw) == (BAD_ARG, "NULL pointer")
    # n < 2 before the residues, the residues before the empty sequence, that before the length
    for seqs in ([], ["AA"], ["AJ"], [""], [too_long]):
        rc, msg = raw_nw(lib, seqs, entry=entry)
        assert rc == BAD_ARG and "need >= 2 sequences" in msg, seqs[:1]
    for seqs, code, text in [(["JA", "AA"], O.ERR_BAD_RES1, "Invalid amino acid in sequence1: J"),
                             (["AJ", "AA"], O.ERR_BAD_RES2, "Invalid amino acid in sequence2: J"),      # pair (1, 1) comes first
                             (["AA", "AJ"], O.ERR_BAD_RES2, "Invalid amino acid in sequence2: J"),
                             (["", "AA", "AJ"], O.ERR_BAD_RES2, "Invalid amino acid in sequence2: J"),
                             ([too_long, "AU"], O.ERR_BAD_RES2, "Invalid amino acid in sequence2: U")]:
        rc, _, message = O.similarity_nw(seqs)
        assert (rc, message) == (code, text), seqs[-1]                                                  # the reference's first-raised message
        assert raw_nw(lib, seqs, entry=entry) == (code, text), seqs[-1]
        assert raw_nw(lib, seqs, entry=entry)[1] == raw_edges_text(lib, seqs)                           # and the edge form's own text
    for seqs in (["AA", ""], ["AA", "", too_long]):
        rc, msg = raw_nw(lib, seqs, entry=entry)
        assert rc == UNSUPPORTED and "sequence 2 is empty" in msg and "NaN" in msg and "median" in msg, msg
    for seqs in ([over, "AA"], ["AA", "AC", over], [too_long, too_long]):
        rc, msg = raw_nw(lib, seqs, entry=entry)
        assert rc == UNSUPPORTED and str(limit) in msg, msg
    fn = da.similarityNW_stats if limit == 127 else da.similarityNW_stats_long
    with pytest.raises(da.DynaAlignError) as ei:
        fn([over, "AA"])
    assert ei.value.code == UNSUPPORTED and str(limit) in str(ei.value)
    # everything in order: the device is asked for last
    assert reaches_the_device(lib, *raw_nw(lib, ["AA", "AC"], entry=entry))
    assert reaches_the_device(lib, *raw_nw(lib, ["A" * limit, "AC"], entry=entry))
    if limit == 1024:
        rc, msg = raw_nw(lib, ["A" * 128, "AC"], entry="da_similarity_nw_stats")
        assert rc == UNSUPPORTED and "127" in msg


def raw_edges_text(lib, seqs):
    res, off = O.pack(seqs)
    h, thr, cnt = ctypes.c_void_p(), ctypes.c_double(), ctypes.c_int64()
    rc = lib.da_similarity_nw_edges_long_begin(res.ctypes.data, off.ctypes.data, len(seqs), b"BLOSUM62", 10, 4, 0.8, ctypes.addressof(h),
                                               ctypes.addressof(thr), ctypes.addressof(cnt))
    assert rc != OK
    return lib.da_last_error().decode("latin-1")


def test_device_entries_check_their_arguments_before_any_pointer(lib):
    p = 4096            # never dereferenced by these

    def ex16(rows=4, n=100, ld=104, keys=p, rank=p, rb=0, cb=0, rec=p):
        return lib.da_dev_upper_extrema(keys, rows, n, ld, rank, rb, cb, rec, None)

    def ex32(rows=4, n=100, ld=104, keys=p, rb=0, cb=0, rec=p, rank=None):
        return lib.da_dev_upper_extrema32(keys, rows, n, ld, rb, cb, rec, None)
    for call in (ex16, ex32):
        assert call(keys=None) == BAD_ARG and call(rec=None) == BAD_ARG
        assert call(ld=99) == BAD_ARG
        assert call(rows=-1) == BAD_ARG and call(n=-1, ld=0) == BAD_ARG
        assert call(rb=-1) == BAD_ARG and call(cb=-1) == BAD_ARG
        assert call(rows=0) == OK and call(rows=0, rb=5, cb=3) == OK and call(rows=0, rank=None) == OK
