"""CPU tests of the long NW threshold boundary (da_similarity_nw_edges_long_begin / da_similarity_nw_cross_edges_long_begin, the device pieces
on 32-bit keys, nw_value_ranks): symbols, Python signatures, the validation order and its texts -- those of the short calls with the one
change that the length refusal is at 1025 residues -- and the value table against Python's fractions.  No compute calls here."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import oracle_lib as O

SYMBOLS = ["da_similarity_nw_edges_long_begin", "da_similarity_nw_cross_edges_long_begin", "da_nw_value_ranks", "da_dev_nw_codes_to_ranks",
           "da_dev_rank_histogram", "da_dev_threshold_ranks_count", "da_dev_threshold_ranks_emit"]
OK, BAD_MATRIX, NO_DEVICE, UNSUPPORTED, BAD_ARG = 0, 4, 8, 10, 11
NAN = float("nan")


@pytest.fixture(scope="module")
def lib(built):
    from dynaalign_amd import _capi
    return _capi.load()


def test_header_library_and_signatures_agree(lib):
    from dynaalign_amd import _capi
    declared = _capi.header_symbols()
    for name in SYMBOLS:
        assert name in declared and name in _capi.SIGNATURES and hasattr(lib, name), name
    assert sorted(_capi.SIGNATURES) == declared
    assert lib.da_abi_version() == 2


def test_python_mirror_exports():
    import inspect
    import dynaalign_amd as da
    from dynaalign_amd import device
    for long_fn, short_fn in ((da.similarityNW_edges_long, da.similarityNW_edges), (da.similarityNW_cross_edges_long, da.similarityNW_cross_edges)):
        assert inspect.signature(long_fn) == inspect.signature(short_fn)
    assert "similarityNW_edges_long" in da.__all__ and "similarityNW_cross_edges_long" in da.__all__ and "nw_value_ranks" in da.__all__
    sig = inspect.signature(da.clusterbreak)
    assert sig.parameters["edges_fn"].default is None and sig.parameters["edges_fn"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(device.nw_codes_to_ranks).parameters) == ["codes", "rank", "max_len", "out"]
    assert list(inspect.signature(device.rank_histogram).parameters) == ["keys", "nbins", "triangle", "row_begin", "col_begin"]
    assert list(inspect.signature(device.threshold_ranks).parameters) == ["keys", "r_min", "nbins", "triangle", "row_begin", "col_begin", "capacity"]


def raw_square(lib, seqs, p, matrix=b"BLOSUM62", entry="da_similarity_nw_edges_long_begin"):
    res, off = O.pack(seqs)
    h, thr, cnt = ctypes.c_void_p(), ctypes.c_double(-7.0), ctypes.c_int64(-7)
    rc = getattr(lib, entry)(res.ctypes.data, off.ctypes.data, len(seqs), matrix, 10, 4, p, ctypes.addressof(h), ctypes.addressof(thr),
                             ctypes.addressof(cnt))
    msg = lib.da_last_error().decode("latin-1") if rc else ""
    if rc == OK:
        assert h.value
        lib.da_edges_free(h)
    else:
        assert not h.value
    return rc, msg


def raw_cross(lib, x, y, thresh, is_q, matrix=b"BLOSUM62", entry="da_similarity_nw_cross_edges_long_begin", want_count=False):
    xr, xo = O.pack(x)
    yr, yo = O.pack(y)
    h, thr, cnt = ctypes.c_void_p(), ctypes.c_double(-7.0), ctypes.c_int64(-7)
    rc = getattr(lib, entry)(xr.ctypes.data, xo.ctypes.data, len(x), yr.ctypes.data, yo.ctypes.data, len(y), matrix, 10, 4, thresh, is_q,
                             ctypes.addressof(h), ctypes.addressof(thr), ctypes.addressof(cnt))
    msg = lib.da_last_error().decode("latin-1") if rc else ""
    if rc == OK:
        assert h.value
        lib.da_edges_free(h)
    if want_count:
        return rc, msg, cnt.value, thr.value
    return rc, msg


def reaches_the_device(lib, rc, msg):
    """valid input: DA_OK where there is a device, DA_ERR_NO_DEVICE -- the last check -- where there is none"""
    if lib.da_device_count() > 0:
        return rc == OK
    return rc == NO_DEVICE and "no CPU fallback" in msg


def test_square_validation_order_and_texts(lib, kats):
    import dynaalign_amd as da
    long_seq = "ACDEFGHIKL" * 103                                                 # 1030 residues
    # the matrix first, whatever else is wrong
    for seqs, p in [(["AA", "AC"], 0.8), (["AA"], 0.8), ([], 0.8), (["AJ", "AA"], 1.5), (["", "AA"], NAN), ([long_seq, "AA"], 0.8)]:
        rc, msg = raw_square(lib, seqs, p, b"PAM250")
        assert (rc, msg) == (BAD_MATRIX, kats["nw_bad_matrix"]["error"]), (seqs[:1], p)
    # n < 2 before thresh_p, thresh_p before the residues, the residues before the empty sequence, that before the length
    for seqs in ([], ["AA"], ["AJ"]):
        for p in (0.8, 1.5, NAN):
            rc, msg = raw_square(lib, seqs, p)
            assert rc == BAD_ARG and "need >= 2 sequences" in msg, (seqs, p)
    for p in (-0.1, 1.5, NAN):
        for seqs in (["AA", "AC"], ["AJ", "AA"], ["", "AA"], [long_seq, "AA"]):
            rc, msg = raw_square(lib, seqs, p)
            assert (rc, msg) == (BAD_ARG, "thresh_p must be in [0, 1]"), (seqs[:1], p)
    for seqs, code, text in [(["JA", "AA"], O.ERR_BAD_RES1, "Invalid amino acid in sequence1: J"),
                             (["AJ", "AA"], O.ERR_BAD_RES2, "Invalid amino acid in sequence2: J"),      # pair (1, 1) comes first
                             (["AA", "AJ"], O.ERR_BAD_RES2, "Invalid amino acid in sequence2: J"),
                             (["", "AA", "AJ"], O.ERR_BAD_RES2, "Invalid amino acid in sequence2: J"),
                             ([long_seq, "AU"], O.ERR_BAD_RES2, "Invalid amino acid in sequence2: U")]:
        rc, _, message = O.similarity_nw(seqs)
        assert (rc, message) == (code, text), seqs[-1]                                                  # the reference's first-raised message
        assert raw_square(lib, seqs, 0.8) == (code, text), seqs[-1]
        assert raw_square(lib, seqs, 0.8, entry="da_similarity_nw_edges_begin") == (code, text), seqs[-1]     # the short call's own text
    for seqs in (["AA", ""], ["AA", "", long_seq]):
        rc, msg = raw_square(lib, seqs, 0.8)
        assert rc == UNSUPPORTED and "sequence 2 is empty" in msg and "NaN" in msg, msg
        assert raw_square(lib, seqs, 0.8, entry="da_similarity_nw_edges_begin") == (rc, msg)
    for seqs in (["A" * 1025, "AA"], ["AA", "AC", "C" * 1025], [long_seq, long_seq]):
        rc, msg = raw_square(lib, seqs, 0.8)
        assert rc == UNSUPPORTED and "1024" in msg, msg
        with pytest.raises(da.DynaAlignError) as ei:
            da.similarityNW_edges_long(seqs)
        assert (ei.value.code, str(ei.value)) == (UNSUPPORTED, msg)
    # the result pointers are needed whatever the input
    res, off = O.pack(["AA", "AC"])
    assert lib.da_similarity_nw_edges_long_begin(res.ctypes.data, off.ctypes.data, 2, b"BLOSUM62", 10, 4, 0.8, None, None, None) == BAD_ARG


def test_128_and_1024_residues_pass_validation_where_the_short_calls_refuse(lib):
    for length in (128, 1024):
        seqs = ["A" * length, "AC"]
        rc, msg = raw_square(lib, seqs, 0.8, entry="da_similarity_nw_edges_begin")
        assert rc == UNSUPPORTED and "127" in msg
        assert reaches_the_device(lib, *raw_square(lib, seqs, 0.8)), length
        for thresh, is_q in ((0.8, 1), (0.5, 0)):
            for x, y in ((seqs[:1], ["AC"]), (["AC"], seqs[:1])):
                rc, msg = raw_cross(lib, x, y, thresh, is_q, entry="da_similarity_nw_cross_edges_begin")
                assert rc == UNSUPPORTED and "127" in msg
                assert reaches_the_device(lib, *raw_cross(lib, x, y, thresh, is_q)), (length, thresh, is_q)


def test_cross_validation_order_and_texts(lib, kats):
    import dynaalign_amd as da
    forms = [(0.8, 1), (-0.1, 1), (1.5, 1), (NAN, 1), (0.5, 0), (NAN, 0)]
    for x, y in [(["AA"], ["AA"]), ([], ["AA"]), (["AA"], []), (["AJ"], ["JJ"]), (["A" * 1025], ["AA"])]:
        for thresh, is_q in forms:
            assert raw_cross(lib, x, y, thresh, is_q, b"PAM250") == (BAD_MATRIX, kats["nw_bad_matrix"]["error"])
    # an empty side: no edges in the absolute form, no quantile in the quantile form
    for x, y in [([], ["AA"]), (["AA"], []), ([], []), ([], ["J"]), ([], ["A" * 1025])]:
        rc, msg, cnt, thr = raw_cross(lib, x, y, 0.25, 0, want_count=True)
        assert (rc, cnt, thr) == (OK, 0, 0.25)
        assert raw_cross(lib, x, y, 0.8, 1) == (BAD_ARG, "quantile of an empty set")
        assert raw_cross(lib, x, y, NAN, 0)[0] == BAD_ARG and raw_cross(lib, x, y, 1.5, 1)[0] == BAD_ARG
    thr, i, j, w = da.similarityNW_cross_edges_long([], ["AA"], threshold=0.5)
    assert thr == 0.5 and i.shape == j.shape == w.shape == (0,) and i.dtype == j.dtype == np.int32 and w.dtype == np.float64
    with pytest.raises(da.DynaAlignError) as ei:
        da.similarityNW_cross_edges_long([], ["AA"], thresh_p=0.8)
    assert (ei.value.code, str(ei.value)) == (BAD_ARG, "quantile of an empty set")
    # the residues (the reference's first-raised message) before the threshold argument, that before the limits on the sequences
    for x, y, code, text in [(["AJ"], ["AA"], O.ERR_BAD_RES1, "Invalid amino acid in sequence1: J"),
                             (["AA"], ["AJ"], O.ERR_BAD_RES2, "Invalid amino acid in sequence2: J"),
                             (["", "JA"], ["AA"], O.ERR_BAD_RES1, "Invalid amino acid in sequence1: J"),
                             (["AA", "AJ"], ["AA", "AU"], O.ERR_BAD_RES2, "Invalid amino acid in sequence2: U")]:
        for thresh, is_q in forms:
            assert raw_cross(lib, x, y, thresh, is_q) == (code, text)
            assert raw_cross(lib, x, y, thresh, is_q, entry="da_similarity_nw_cross_edges_begin") == (code, text)
    for thresh, is_q in [(-0.1, 1), (1.5, 1), (NAN, 1), (NAN, 0)]:
        for x in (["AA"], ["AA", ""], ["A" * 1025]):
            assert raw_cross(lib, x, ["AA"], thresh, is_q)[0] == BAD_ARG
    for thresh, is_q in [(0.8, 1), (0.5, 0)]:
        for x, y, who in [(["AA", ""], ["AA"], "sequence 2 of x"), (["AA"], ["AC", "AA", ""], "sequence 3 of y")]:
            rc, msg = raw_cross(lib, x, y, thresh, is_q)
            assert rc == UNSUPPORTED and who in msg and "empty" in msg and "quantile" in msg, msg
            assert raw_cross(lib, x, y, thresh, is_q, entry="da_similarity_nw_cross_edges_begin") == (rc, msg)
        for x, y in ((["A" * 1025], ["AA"]), (["AA"], ["AC", "A" * 1025])):
            rc, msg = raw_cross(lib, x, y, thresh, is_q)
            assert rc == UNSUPPORTED and "1024" in msg, msg


def test_piece_calls_check_their_arguments_before_any_pointer(lib):
    p = 4096            # never dereferenced by these

    def to_ranks(rows=4, n=100, ld=104, max_len=50, codes=p, rank=p, out=p, ld_out=104):
        return lib.da_dev_nw_codes_to_ranks(codes, rows, n, ld, max_len, rank, out, ld_out, None)

    def hist(rows=4, n=100, ld=104, nbins=501, keys=p, out=p, tri=0, rb=0, cb=0):
        return lib.da_dev_rank_histogram(keys, rows, n, ld, nbins, out, tri, rb, cb, None)

    def count(rows=4, n=100, ld=104, nbins=501, keys=p, rowptr=p, work=p, tri=0, rb=0, cb=0):
        return lib.da_dev_threshold_ranks_count(keys, rows, n, ld, 1, nbins, tri, rb, cb, rowptr, work, 1 << 20, None)

    def emit(rows=4, n=100, ld=104, nbins=501, keys=p, rowptr=p, j=p, key=p, cap=10, tri=0, rb=0, cb=0):
        return lib.da_dev_threshold_ranks_emit(keys, rows, n, ld, 1, nbins, tri, rb, cb, rowptr, j, key, cap, None)
    for call in (hist, count, emit):
        assert call(ld=99) == BAD_ARG and call(nbins=0) == BAD_ARG and call(nbins=1 << 31) == BAD_ARG and call(nbins=-1) == BAD_ARG
        assert call(keys=None) == BAD_ARG
        assert call(rows=-1) == BAD_ARG and call(n=-1, ld=0) == BAD_ARG
        assert call(tri=1, rb=-1) == BAD_ARG and call(tri=1, cb=-1) == BAD_ARG
        assert call(rows=0) == OK and call(rows=0, nbins=1301496, tri=1, rb=5, cb=3) == OK
    assert hist(out=None) == BAD_ARG
    assert count(rowptr=None) == BAD_ARG and count(work=None) == BAD_ARG
    assert emit(rowptr=None) == BAD_ARG and emit(j=None) == BAD_ARG and emit(key=None) == BAD_ARG and emit(cap=-1) == BAD_ARG
    assert to_ranks(codes=None) == BAD_ARG and to_ranks(rank=None) == BAD_ARG and to_ranks(out=None) == BAD_ARG
    assert to_ranks(ld=99) == BAD_ARG and to_ranks(ld_out=99) == BAD_ARG and to_ranks(max_len=0) == BAD_ARG and to_ranks(max_len=1025) == BAD_ARG
    assert to_ranks(rows=0) == OK and to_ranks(rows=-1) == BAD_ARG


# ---- the value table ------------------------------------------------------------------------------------------------------------------------------

def domain(max_len):
    return [(ln, mt) for ln in range(1, 2 * max_len + 1) for mt in range(0, min(ln, max_len) + 1)]


def test_value_ranks_arguments(lib):
    d = ctypes.c_int64(-7)
    out = np.zeros(64, np.float64)
    assert lib.da_nw_value_ranks(0, None, ctypes.addressof(d), None) == BAD_ARG
    assert lib.da_nw_value_ranks(1025, None, ctypes.addressof(d), None) == BAD_ARG
    assert lib.da_nw_value_ranks(5, None, None, None) == BAD_ARG
    assert lib.da_nw_value_ranks(5, out.ctypes.data, ctypes.addressof(d), None) == BAD_ARG       # one output without the other
    assert lib.da_nw_value_ranks(1, None, ctypes.addressof(d), None) == OK and d.value == 3      # 0, 1/2, 1


@pytest.mark.parametrize("max_len", [1, 2, 3, 40])
def test_value_ranks_against_fractions(max_len):
    from dynaalign_amd import nw_value_ranks
    values, rank = nw_value_ranks(max_len)
    assert values.dtype == np.float64 and rank.dtype == np.uint32 and rank.shape == (2 * max_len + 1, max_len + 1)
    fr = sorted({Fraction(mt, ln) for ln, mt in domain(max_len)})
    assert np.array_equal(values.view(np.uint64), np.array([f.numerator / f.denominator for f in fr], np.float64).view(np.uint64))
    index = {f: r for r, f in enumerate(fr)}
    for ln, mt in domain(max_len):
        assert rank[ln, mt] == index[Fraction(mt, ln)], (ln, mt)
    inside = np.zeros(rank.shape, bool)
    for ln, mt in domain(max_len):
        inside[ln, mt] = True
    assert (rank[~inside] == 0).all()                                             # length 0, matches > length


def test_value_ranks_127_order_the_codes_as_nw_code_ranks_does():
    from dynaalign_amd import nw_code_ranks, nw_value_ranks
    values, rank = nw_value_ranks(127)
    old, distinct = nw_code_ranks(127)
    assert len(values) == distinct
    ln, mt = np.array(domain(127)).T
    assert np.array_equal(rank[ln, mt], old[(mt << 8) | ln])                      # both dense from 0: the same order, the same ties


def test_value_ranks_1024():
    from dynaalign_amd import nw_value_ranks
    values, rank = nw_value_ranks(1024)
    # distinct reduced fractions p / q in [0, 1] that SOME pair of the domain reduces to: q <= 2048 and p <= 1024 (mt = p, ln = q itself is in
    # the domain; and any pair that reduces to p / q has p <= mt <= 1024)
    q, p_ = np.arange(1, 2049)[:, None], np.arange(0, 1025)[None, :]
    want = int(((np.gcd(p_, q) == 1) & (p_ <= q)).sum())
    assert want == sum(1 for b in range(1, 41) for a in range(0, b + 1) if Fraction(a, b).denominator == b) + int(
        ((np.gcd(p_, q) == 1) & (p_ <= q) & (q > 40)).sum())                     # the vectorised count agrees with fractions on q <= 40
    assert len(values) == want
    assert values[0] == 0.0 and values[-1] == 1.0 and (np.diff(values) > 0).all()
    ln = np.arange(1, 2049)[:, None]
    mt = np.arange(0, 1025)[None, :]
    inside = np.broadcast_to(mt <= ln, (2048, 1025))
    r = rank[1:]
    assert ((r == 0) == (np.broadcast_to(mt == 0, r.shape) | ~inside)).all()      # rank 0 <=> matches == 0 inside the domain
    assert np.array_equal(values[r[inside]].view(np.uint64), (mt / ln)[inside].view(np.uint64))   # values[rank] is the divide, bit for bit
    assert rank[256, 128] == rank[300, 150] == rank[2, 1] and values[rank[256, 128]] == 0.5
    assert rank[2048, 1024] == rank[2, 1] and rank[1024, 1024] == len(values) - 1
