"""CPU tests of the two-set threshold boundary (similarityMH_cross_edges / similarityNW_cross_edges, the one-call device route,
da_dev_rect_histogram and da_dev_threshold_rows_*): symbols, Python signatures, validation order and texts (those of the *_cross calls,
then the threshold argument, then the NW limits of the top-k call).  No compute calls here."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O

EDGE_SYMBOLS = ["da_similarity_mh_cross_edges_begin", "da_similarity_nw_cross_edges_begin", "da_dev_similarity_mh_cross_edges",
                "da_dev_rect_histogram", "da_dev_threshold_rows_workspace_bytes", "da_dev_threshold_rows_count", "da_dev_threshold_rows_emit"]
OK, EMPTY, BAD_K, BAD_NHASH, BAD_MATRIX, NO_DEVICE, UNSUPPORTED, BAD_ARG = 0, 1, 2, 3, 4, 8, 10, 11
NAN = float("nan")


@pytest.fixture(scope="module")
def lib(built):
    from dynaalign_amd import _capi
    return _capi.load()


def test_header_library_and_signatures_agree_on_the_edge_symbols(lib):
    from dynaalign_amd import _capi
    declared = _capi.header_symbols()
    for name in EDGE_SYMBOLS:
        assert name in declared, name
        assert name in _capi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert sorted(_capi.SIGNATURES) == declared
    assert lib.da_abi_version() == 2


def test_python_mirror_exports():
    import inspect
    import dynaalign_amd as da
    from dynaalign_amd import device, session
    sig = inspect.signature(da.similarityMH_cross_edges)
    assert list(sig.parameters) == ["x", "y", "k", "n_hash", "thresh_p", "threshold", "seed"]
    assert [sig.parameters[p].default for p in ("k", "n_hash", "thresh_p", "threshold", "seed")] == [4, 50, 0.8, None, None]
    assert sig.parameters["threshold"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["seed"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(da.similarityNW_cross_edges)
    assert list(sig.parameters) == ["x", "y", "matrixName", "gapOpen", "gapExt", "thresh_p", "threshold"]
    assert [sig.parameters[p].default for p in ("matrixName", "gapOpen", "gapExt", "thresh_p", "threshold")] == ["BLOSUM62", 10, 4, 0.8, None]
    assert sig.parameters["threshold"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(device.rect_histogram).parameters) == ["keys", "nbins"]
    sig = inspect.signature(device.threshold_rows)
    assert list(sig.parameters) == ["keys", "keep", "capacity"] and sig.parameters["capacity"].default is None
    sig = inspect.signature(device.similarity_mh_cross_edges)
    assert list(sig.parameters) == ["dx", "dy", "k", "n_hash", "seeds", "thresh_p", "threshold", "capacity"]
    assert [sig.parameters[p].default for p in ("thresh_p", "threshold", "capacity")] == [None, None, None]
    sig = inspect.signature(session.MinHashSession.cross_edges)
    assert list(sig.parameters)[:5] == ["self", "sequences", "thresh_p", "threshold", "idx"]
    assert [sig.parameters[p].default for p in ("thresh_p", "threshold", "idx")] == [0.8, None, None]


def raw_mh(lib, x, y, k, nh, thresh, is_q):
    xr, xo = O.pack(x)
    yr, yo = O.pack(y)
    seeds = np.zeros(max(nh, 1), np.uint32)
    h, thr, cnt = ctypes.c_void_p(), ctypes.c_double(-7.0), ctypes.c_int64(-7)
    rc = lib.da_similarity_mh_cross_edges_begin(xr.ctypes.data, xo.ctypes.data, len(x), yr.ctypes.data, yo.ctypes.data, len(y), k, nh,
                                                seeds.ctypes.data, thresh, is_q, ctypes.addressof(h), ctypes.addressof(thr), ctypes.addressof(cnt))
    msg = lib.da_last_error().decode("latin-1") if rc else ""
    if rc == OK:
        assert h.value
        lib.da_edges_free(h)
    else:
        assert not h.value
    return rc, msg


def raw_nw(lib, x, y, thresh, is_q, matrix=b"BLOSUM62", want_count=False):
    xr, xo = O.pack(x)
    yr, yo = O.pack(y)
    h, thr, cnt = ctypes.c_void_p(), ctypes.c_double(-7.0), ctypes.c_int64(-7)
    rc = lib.da_similarity_nw_cross_edges_begin(xr.ctypes.data, xo.ctypes.data, len(x), yr.ctypes.data, yo.ctypes.data, len(y), matrix, 10, 4,
                                                thresh, is_q, ctypes.addressof(h), ctypes.addressof(thr), ctypes.addressof(cnt))
    msg = lib.da_last_error().decode("latin-1") if rc else ""
    if rc == OK:
        assert h.value
        lib.da_edges_free(h)
    if want_count:
        return rc, msg, cnt.value, thr.value
    return rc, msg


THRESHOLD_ARGS = [(0.8, 1), (-0.1, 1), (1.5, 1), (NAN, 1), (0.5, 0), (NAN, 0)]       # valid and invalid alike: what comes first wins


def test_mh_validation_is_that_of_the_cross_call_then_the_threshold(lib, kats):
    import dynaalign_amd as da
    e = kats["mh_errors"]
    for x, y, k, nh, code, msg in [([], [], 0, 0, EMPTY, e["empty"]), ([], ["ACDE"], 0, 0, EMPTY, e["empty"]), (["ACDE"], [], 0, 0, EMPTY, e["empty"]),
                                   (["ACDE"], ["ACDE"], 0, 0, BAD_K, e["k"]), (["ACDE"], ["ACDE"], -1, 5, BAD_K, e["k"]),
                                   (["ACDE"], ["ACDE"], 4, 0, BAD_NHASH, e["n_hash"]), (["ACDE"], ["ACDE"], 4, -3, BAD_NHASH, e["n_hash"])]:
        with pytest.raises(da.DynaAlignError) as ej:
            da.similarityMH_cross(x, y, k, nh)
        assert (ej.value.code, str(ej.value)) == (code, msg)
        for thresh, is_q in THRESHOLD_ARGS:
            assert raw_mh(lib, x, y, k, nh, thresh, is_q) == (code, msg), (x, y, k, nh, thresh, is_q)
            with pytest.raises(da.DynaAlignError) as ei:
                if is_q:
                    da.similarityMH_cross_edges(x, y, k, nh, thresh)
                else:
                    da.similarityMH_cross_edges(x, y, k, nh, threshold=thresh)
            assert (ei.value.code, str(ei.value)) == (code, msg), (x, y, k, nh, thresh, is_q)
    # then the threshold argument
    for p in (-0.1, 1.5, NAN):
        assert raw_mh(lib, ["ACDE"], ["ACDE"], 4, 8, p, 1)[0] == BAD_ARG
        with pytest.raises(da.DynaAlignError) as ei:
            da.similarityMH_cross_edges(["ACDE"], ["ACDE"], 4, 8, p, seed=1)
        assert ei.value.code == BAD_ARG
    assert raw_mh(lib, ["ACDE"], ["ACDE"], 4, 8, NAN, 0)[0] == BAD_ARG
    with pytest.raises(da.DynaAlignError) as ei:
        da.similarityMH_cross_edges(["ACDE"], ["ACDE"], 4, 8, threshold=NAN, seed=1)
    assert ei.value.code == BAD_ARG
    # the 16-bit limit comes before the threshold check, as in the cross call it comes before the device
    for thresh, is_q in THRESHOLD_ARGS:
        assert raw_mh(lib, ["ACDE"], ["ACDE"], 4, 70000, thresh, is_q)[0] == UNSUPPORTED
    # the result pointers are needed whatever the input
    xr, xo = O.pack(["ACDE"])
    assert lib.da_similarity_mh_cross_edges_begin(xr.ctypes.data, xo.ctypes.data, 1, xr.ctypes.data, xo.ctypes.data, 1, 4, 8, xr.ctypes.data, 0.5, 0,
                                                  None, None, None) == BAD_ARG


def test_device_one_call_validates_alike_before_it_looks_at_a_pointer(lib):
    def dev(m, n, k, nh, thresh=0.5, is_q=0, p=None, cap=0, outs=None):
        return lib.da_dev_similarity_mh_cross_edges(p, p, m, p, p, n, k, nh, p, thresh, is_q, p, p, p, cap, outs, outs, None)
    for m, n, k, nh, code in [(0, 0, 0, 0, EMPTY), (0, 3, 4, 8, EMPTY), (3, 0, 4, 8, EMPTY), (3, 3, 0, 0, BAD_K), (3, 3, 4, 0, BAD_NHASH)]:
        for thresh, is_q in THRESHOLD_ARGS:
            assert dev(m, n, k, nh, thresh, is_q) == code
    assert dev(3, 3, 4, 8) == BAD_ARG                                        # NULL pointers
    host = (ctypes.c_double * 2)()
    p, outs = 4096, ctypes.addressof(host)
    assert dev(3, 3, 4, 70000, NAN, 0, p, 0, outs) == UNSUPPORTED            # the 16-bit limit before the threshold
    for thresh, is_q in [(-0.1, 1), (1.5, 1), (NAN, 1), (NAN, 0)]:
        assert dev(3, 3, 4, 8, thresh, is_q, p, 0, outs) == BAD_ARG
    assert dev(3, 3, 4, 8, 0.5, 0, p, -1, outs) == BAD_ARG


def test_nw_validation(lib, kats):
    import dynaalign_amd as da
    # the matrix first, whatever else is wrong
    for x, y in [(["AA"], ["AA"]), ([], ["AA"]), (["AA"], []), (["AJ"], ["JJ"])]:
        for thresh, is_q in THRESHOLD_ARGS:
            with pytest.raises(da.DynaAlignError) as ei:
                if is_q:
                    da.similarityNW_cross_edges(x, y, "PAM250", thresh_p=thresh)
                else:
                    da.similarityNW_cross_edges(x, y, "PAM250", threshold=thresh)
            assert (ei.value.code, str(ei.value)) == (BAD_MATRIX, kats["nw_bad_matrix"]["error"])
    # an empty side: no edges in the absolute form, no quantile in the quantile form
    for x, y in [([], ["AA"]), (["AA"], []), ([], []), ([], ["J"])]:
        rc, msg, cnt, thr = raw_nw(lib, x, y, 0.25, 0, want_count=True)
        assert (rc, cnt, thr) == (OK, 0, 0.25)
        rc, msg = raw_nw(lib, x, y, 0.8, 1)
        assert rc == BAD_ARG and msg == "quantile of an empty set"
    thr, i, j, w = da.similarityNW_cross_edges([], ["AA"], threshold=0.5)
    assert thr == 0.5 and i.shape == j.shape == w.shape == (0,) and i.dtype == j.dtype == np.int32 and w.dtype == np.float64
    # residue errors are those of da_similarity_nw_cross, unchanged, and come before the threshold check and the empty-sequence refusal
    for x, y, code, msg in [(["AJ"], ["AA"], O.ERR_BAD_RES1, "Invalid amino acid in sequence1: J"),
                            (["AA"], ["AJ"], O.ERR_BAD_RES2, "Invalid amino acid in sequence2: J"),
                            (["", "JA"], ["AA"], O.ERR_BAD_RES1, "Invalid amino acid in sequence1: J"),
                            (["A"], ["J", "AA"], O.ERR_BAD_RES2, "Invalid amino acid in sequence2: J"),
                            (["AA", "AJ"], ["AA", "AU"], O.ERR_BAD_RES2, "Invalid amino acid in sequence2: U")]:
        with pytest.raises(da.DynaAlignError) as ei:
            da.similarityNW_cross(x, y)
        assert (ei.value.code, str(ei.value)) == (code, msg)
        for thresh, is_q in THRESHOLD_ARGS:
            assert raw_nw(lib, x, y, thresh, is_q) == (code, msg), (x, y, thresh, is_q)
    # then the threshold argument, before the limits on the sequences
    for thresh, is_q in [(-0.1, 1), (1.5, 1), (NAN, 1), (NAN, 0)]:
        assert raw_nw(lib, ["AA"], ["AA"], thresh, is_q)[0] == BAD_ARG
        assert raw_nw(lib, ["AA", ""], ["AA"], thresh, is_q)[0] == BAD_ARG
    # an empty sequence on either side is refused with a message; so is a sequence beyond the 8-bit alignment length
    for thresh, is_q in [(0.8, 1), (0.5, 0)]:
        for x, y, who in [(["AA", ""], ["AA"], "sequence 2 of x"), (["AA"], ["AC", "AA", ""], "sequence 3 of y")]:
            rc, msg = raw_nw(lib, x, y, thresh, is_q)
            assert rc == UNSUPPORTED and who in msg and "empty" in msg and "NaN" in msg and "quantile" in msg, msg
        rc, msg = raw_nw(lib, ["A" * 128], ["AA"], thresh, is_q)
        assert rc == UNSUPPORTED and "127" in msg
        rc, msg = raw_nw(lib, ["AA"], ["A" * 128], thresh, is_q)
        assert rc == UNSUPPORTED and "127" in msg


def test_piece_calls_check_their_arguments_before_any_pointer(lib):
    p = 4096            # never dereferenced by these

    def hist(rows=4, n=100, ld=104, nbins=501, keys=p, out=p):
        return lib.da_dev_rect_histogram(keys, rows, n, ld, nbins, out, None)

    def count(rows=4, n=100, ld=104, nbins=501, keys=p, keep=p, rowptr=p, work=p):
        return lib.da_dev_threshold_rows_count(keys, rows, n, ld, keep, nbins, rowptr, work, 1 << 20, None)

    def emit(rows=4, n=100, ld=104, nbins=501, keys=p, keep=p, rowptr=p, j=p, key=p, cap=10):
        return lib.da_dev_threshold_rows_emit(keys, rows, n, ld, keep, nbins, rowptr, j, key, cap, None)
    for call in (hist, count, emit):
        assert call(ld=99) == BAD_ARG and call(nbins=0) == BAD_ARG and call(nbins=65537) == BAD_ARG and call(nbins=-1) == BAD_ARG
        assert call(keys=None) == BAD_ARG
        assert call(rows=-1) == BAD_ARG and call(n=-1, ld=0) == BAD_ARG
        assert call(rows=0) == OK
        assert call(rows=0, nbins=65536) == OK
    assert hist(out=None) == BAD_ARG
    assert count(keep=None) == BAD_ARG and count(rowptr=None) == BAD_ARG and count(work=None) == BAD_ARG
    assert emit(keep=None) == BAD_ARG and emit(rowptr=None) == BAD_ARG and emit(j=None) == BAD_ARG and emit(key=None) == BAD_ARG
    assert emit(cap=-1) == BAD_ARG
    # NULL comes before the other checks
    assert hist(keys=None, ld=99) == BAD_ARG and count(keep=None, nbins=0) == BAD_ARG
    assert lib.da_dev_threshold_rows_workspace_bytes(0) > 0
    assert lib.da_dev_threshold_rows_workspace_bytes(1000) >= 1001 * 8


def test_valid_input_fails_loudly_without_a_device(lib):
    x, y = ["ACDEFG", "ACDEFH"], ["ACDEFG", "ACDEFH", "ACDEFI"]
    calls = [lambda: raw_mh(lib, x, y, 4, 8, 0.5, 0), lambda: raw_mh(lib, x, y, 4, 8, 0.8, 1),
             lambda: raw_nw(lib, ["ACD", "AC"], ["AC", "A"], 0.5, 0), lambda: raw_nw(lib, ["ACD", "AC"], ["AC", "A"], 0.8, 1)]
    if lib.da_device_count() > 0:
        for call in calls:
            assert call()[0] == OK
        return
    for call in calls:
        rc, msg = call()
        assert rc == NO_DEVICE and "no CPU fallback" in msg
