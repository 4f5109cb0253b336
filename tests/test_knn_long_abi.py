"""CPU tests of the nearest-neighbour / top-k boundary for sequences of up to 1024 residues (da_similarity_nw_knn_long,
da_similarity_nw_cross_topk_long, da_dev_topk_ranks, da_dev_topk_ranks_self): symbols, the Python mirror's signatures, and the validation
order and texts, which are those of the short calls apart from the length refusal -- every error arrives before a device is needed.  No
compute calls here."""
import inspect

import numpy as np
import pytest

import oracle_lib as O

SYMBOLS = ["da_similarity_nw_knn_long", "da_similarity_nw_cross_topk_long", "da_dev_topk_ranks", "da_dev_topk_ranks_self"]
OK, BAD_MATRIX, NO_DEVICE, UNSUPPORTED, BAD_ARG = 0, 4, 8, 10, 11
SECOND = "a nearest neighbour needs a second sequence"
TOP_TEXT = "top-k per row keeps its candidates in a fixed LDS buffer: top <= 1024 (got 1025)"


@pytest.fixture(scope="module")
def lib(built):
    from dynaalign_amd import _capi
    return _capi.load()


def test_header_library_and_signatures_agree_on_the_new_symbols(lib):
    from dynaalign_amd import _capi
    declared = _capi.header_symbols()
    for name in SYMBOLS:
        assert name in declared, name
        assert name in _capi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert sorted(_capi.SIGNATURES) == declared
    assert lib.da_abi_version() == 2


def test_python_mirror_exports():
    import dynaalign_amd as da
    from dynaalign_amd import device
    for name in ("similarityNW_knn_long", "similarityNW_knn_edges_long", "similarityNW_cross_topk_long"):
        assert name in da.__all__ and callable(getattr(da, name)), name
    sig = inspect.signature(da.similarityNW_knn_long)
    assert list(sig.parameters) == ["sequences", "matrixName", "gapOpen", "gapExt", "top"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == ["BLOSUM62", 10, 4, 10]
    assert sig == inspect.signature(da.similarityNW_knn)
    sig = inspect.signature(da.similarityNW_knn_edges_long)
    assert list(sig.parameters) == ["sequences", "matrixName", "gapOpen", "gapExt", "top", "mode"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == ["BLOSUM62", 10, 4, 10, "union"]
    assert sig == inspect.signature(da.similarityNW_knn_edges)
    sig = inspect.signature(da.similarityNW_cross_topk_long)
    assert list(sig.parameters) == ["x", "y", "matrixName", "gapOpen", "gapExt", "top"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == ["BLOSUM62", 10, 4, 10]
    assert sig == inspect.signature(da.similarityNW_cross_topk)
    sig = inspect.signature(device.topk_ranks)
    assert list(sig.parameters) == ["keys", "top", "nbins", "self_col0", "want_self"]
    assert sig.parameters["self_col0"].default is None and sig.parameters["want_self"].default is False


def raw_knn(lib, seqs, top, matrix=b"BLOSUM62", with_val=True, with_diag=True, entry="da_similarity_nw_knn_long"):
    res, off = O.pack(seqs)
    cnt = max(len(seqs), 1) * max(top, 1)
    idx, val, diag = np.full(cnt, -7, np.int32), np.full(cnt, -7.0), np.full(max(len(seqs), 1), -7.0)
    rc = getattr(lib, entry)(res.ctypes.data, off.ctypes.data, len(seqs), matrix, 10, 4, top, idx.ctypes.data, val.ctypes.data if with_val else None,
                             diag.ctypes.data if with_diag else None)
    return rc, lib.da_last_error().decode("latin-1") if rc else ""


def raw_cross(lib, x, y, top, matrix=b"BLOSUM62", with_val=True, with_idx=True, entry="da_similarity_nw_cross_topk_long"):
    xr, xo = O.pack(x)
    yr, yo = O.pack(y)
    cnt = max(len(x), 1) * max(top, 1)
    idx, val = np.full(cnt, -7, np.int32), np.full(cnt, -7.0)
    rc = getattr(lib, entry)(xr.ctypes.data, xo.ctypes.data, len(x), yr.ctypes.data, yo.ctypes.data, len(y), matrix, 10, 4, top,
                             idx.ctypes.data if with_idx else None, val.ctypes.data if with_val else None)
    return rc, lib.da_last_error().decode("latin-1") if rc else ""


def test_one_set_validation_is_that_of_the_short_call(lib, kats):
    import dynaalign_amd as da
    for seqs in (["AA", "AC"], [], ["AJ", "JJ"], ["AA"]):                          # the matrix name first
        with pytest.raises(da.DynaAlignError) as ei:
            da.similarityNW_knn_long(seqs, "PAM250")
        assert (ei.value.code, str(ei.value)) == (BAD_MATRIX, kats["nw_bad_matrix"]["error"])
        with pytest.raises(da.DynaAlignError) as ei:
            da.similarityNW_knn_edges_long(seqs, "PAM250")
        assert ei.value.code == BAD_MATRIX
        assert raw_knn(lib, seqs, 1, b"PAM250")[0] == BAD_MATRIX
    for seqs in ([], ["AA"], ["AJ"]):                                              # a second sequence before anything about the residues
        assert raw_knn(lib, seqs, 1) == (BAD_ARG, SECOND)
    for top in (0, -1, 2, 3):                                                      # top before the residues; not clamped
        rc, msg = raw_knn(lib, ["AA", "AJ"], top)
        assert rc == BAD_ARG and "top must be in 1 .. n - 1" in msg
        assert (rc, msg) == raw_knn(lib, ["AA", "AJ"], top, entry="da_similarity_nw_knn")
    assert raw_knn(lib, ["AA"] * 1027, 1025) == (UNSUPPORTED, TOP_TEXT)
    # every text up to the length refusal is the short call's
    cases = [["JA", "AA"], ["AJ", "AA"], ["AA", "AJ"], ["AA", "AC", "AU"], ["AA", "", "AC"], ["AA", "", "AJ"]]
    want = [(O.ERR_BAD_RES1, "Invalid amino acid in sequence1: J"), (O.ERR_BAD_RES2, "Invalid amino acid in sequence2: J"),
            (O.ERR_BAD_RES2, "Invalid amino acid in sequence2: J"), (O.ERR_BAD_RES2, "Invalid amino acid in sequence2: U")]
    for t, seqs in enumerate(cases):
        got = raw_knn(lib, seqs, 1)
        assert got == raw_knn(lib, seqs, 1, entry="da_similarity_nw_knn"), seqs
        if t < len(want):
            assert got == want[t], seqs
    rc, msg = raw_knn(lib, ["AA", "", "AC"], 1)
    assert rc == UNSUPPORTED and "sequence 2 is empty" in msg and "NaN" in msg
    # the one difference: 1024 residues, not 127; after the residues and the empty sequence
    rc, msg = raw_knn(lib, ["A" * 1025, "AA"], 1)
    assert rc == UNSUPPORTED and "1024" in msg and "32-bit value ranks" in msg
    assert raw_knn(lib, ["A" * 1025, "AJ"], 1)[0] == O.ERR_BAD_RES2
    assert raw_knn(lib, ["A" * 1025, ""], 1)[0] == UNSUPPORTED and "empty" in raw_knn(lib, ["A" * 1025, ""], 1)[1]
    with pytest.raises(da.DynaAlignError) as ei:
        da.similarityNW_knn_long(["A" * 1025, "AA"])
    assert ei.value.code == UNSUPPORTED and "1024" in str(ei.value)
    rc, msg = raw_knn(lib, ["A" * 128, "AA"], 1, entry="da_similarity_nw_knn")      # the short call is unchanged
    assert rc == UNSUPPORTED and "127" in msg
    res, off = O.pack(["AA", "AC"])
    idx = np.zeros(2, np.int32)
    assert lib.da_similarity_nw_knn_long(None, off.ctypes.data, 2, b"BLOSUM62", 10, 4, 1, idx.ctypes.data, None, None) == BAD_ARG
    assert lib.da_similarity_nw_knn_long(res.ctypes.data, off.ctypes.data, 2, b"BLOSUM62", 10, 4, 1, None, None, None) == BAD_ARG


def test_two_set_validation_is_that_of_the_short_call(lib, kats):
    import dynaalign_amd as da
    with pytest.raises(da.DynaAlignError) as ei:
        da.similarityNW_cross_topk_long(["AA"], ["AC"], "PAM250")
    assert (ei.value.code, str(ei.value)) == (BAD_MATRIX, kats["nw_bad_matrix"]["error"])
    assert raw_cross(lib, [], [], 1, b"PAM250")[0] == BAD_MATRIX
    assert raw_cross(lib, [], ["AA"], 1)[0] == OK and raw_cross(lib, [], [], 0)[0] == OK      # no rows: nothing to write
    cases = [(["AA"], [], 1), (["AA"], ["AC"], 0), (["AA"], ["AC"], 2), (["AA"], ["AC", "AD"], 3), (["JA"], ["AA"], 1), (["AA"], ["AJ"], 1),
             (["AA"], ["AJ"], 5), (["AA", ""], ["AC"], 1), (["AA"], ["AC", ""], 1), (["AA"], ["AA"] * 1027, 1025), (["AA"], ["AA"] * 1027, 1028)]
    for x, y, top in cases:
        got = raw_cross(lib, x, y, top)
        assert got[0] != OK and got == raw_cross(lib, x, y, top, entry="da_similarity_nw_cross_topk"), (x[:2], y[:2], top)
    assert raw_cross(lib, ["AA"], [], 1)[0] == BAD_ARG and "n = 0" in raw_cross(lib, ["AA"], [], 1)[1]
    assert raw_cross(lib, ["AA"], ["AA"] * 1027, 1025) == (UNSUPPORTED, TOP_TEXT)
    assert raw_cross(lib, ["AA"], ["AC"], 1, with_idx=False)[0] == BAD_ARG
    rc, msg = raw_cross(lib, ["AA", ""], ["AC"], 1)
    assert rc == UNSUPPORTED and "sequence 2 of x is empty" in msg
    for x, y in ((["A" * 1025], ["AA"]), (["AA"], ["AC", "A" * 1025])):
        rc, msg = raw_cross(lib, x, y, 1)
        assert rc == UNSUPPORTED and "1024" in msg and "32-bit value ranks" in msg
    assert raw_cross(lib, ["A" * 1025], ["AJ"], 1)[0] == O.ERR_BAD_RES2
    rc, msg = raw_cross(lib, ["A" * 128], ["AA"], 1, entry="da_similarity_nw_cross_topk")
    assert rc == UNSUPPORTED and "127" in msg


def test_the_selection_on_ranks_checks_its_arguments_before_a_device(lib):
    p = 4096

    def plain(rows=4, n=100, ld=104, nbins=1000, top=10, ld_out=10, keys=p, idx=p, key=p):
        return lib.da_dev_topk_ranks(keys, rows, n, ld, nbins, top, idx, key, ld_out, None)

    def own(rows=4, n=100, ld=104, nbins=1000, top=10, ld_out=10, keys=p, idx=p, key=p, col0=0):
        return lib.da_dev_topk_ranks_self(keys, rows, n, ld, nbins, top, col0, idx, key, ld_out, None, None)
    for f in (plain, own):
        assert f(top=0) == BAD_ARG and f(top=101) == BAD_ARG and f(ld=99) == BAD_ARG and f(ld_out=9) == BAD_ARG
        assert f(keys=None) == BAD_ARG and f(idx=None) == BAD_ARG and f(key=None) == BAD_ARG
        assert f(nbins=0) == BAD_ARG and "nbins must be in 1 .. 2^31 - 1" in lib.da_last_error().decode()
        assert f(nbins=1 << 31) == BAD_ARG and "nbins must be in 1 .. 2^31 - 1" in lib.da_last_error().decode()
        assert f(n=2000, ld=2000, top=1025, ld_out=1025) == UNSUPPORTED and lib.da_last_error().decode() == TOP_TEXT
        assert f(rows=0) == OK and f(rows=-1) == BAD_ARG
    assert own(top=100) == BAD_ARG and "1 .. n - 1" in lib.da_last_error().decode()           # top = n only through the plain form
    assert plain(top=100, ld_out=99) == BAD_ARG and "ld_out" in lib.da_last_error().decode()  # ... which accepts it and looks at ld_out


def test_python_mirror_clamps_top_and_valid_input_fails_loudly_without_a_device(lib):
    import dynaalign_amd as da
    seqs = ["ACDEFG", "ACDEFH", "A" * 128]                                          # 128 residues: accepted up to the device check
    calls = (lambda: da.similarityNW_knn_long(seqs, top=9), lambda: da.similarityNW_cross_topk_long(seqs, seqs[:2], top=9))
    for call in calls:
        if lib.da_device_count() > 0:
            idx, val = call()
            assert idx.shape == (3, 2) and val.shape == (3, 2) and idx.dtype == np.int32 and val.dtype == np.float64
        else:
            with pytest.raises(da.DynaAlignError) as ei:
                call()
            assert ei.value.code == NO_DEVICE and "no CPU fallback" in str(ei.value)
    if lib.da_device_count() > 0:
        thr, i, j, w = da.similarityNW_knn_edges_long(seqs, top=9)
        assert i.dtype == np.int32 and len(i) == len(j) == len(w) >= 3
    want = OK if lib.da_device_count() > 0 else NO_DEVICE
    assert raw_knn(lib, seqs, 2)[0] == want and raw_knn(lib, seqs, 2, with_val=False, with_diag=False)[0] == want
    assert raw_cross(lib, seqs, seqs, 3)[0] == want and raw_cross(lib, seqs, seqs, 3, with_val=False)[0] == want
    assert da.similarityNW_cross_topk_long([], seqs, top=2)[0].shape == (0, 2)
