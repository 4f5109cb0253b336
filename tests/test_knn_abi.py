"""CPU tests of the one-set nearest-neighbour boundary (da_similarity_mh_knn / da_similarity_nw_knn, da_dev_similarity_mh_knn,
da_dev_topk_rows_self, da_dev_knn_edges): symbols, the Python mirror's signatures, and the validation order and texts -- every error
arrives before a device is needed.  No compute calls here."""
import inspect

import numpy as np
import pytest

import oracle_lib as O

KNN_SYMBOLS = ["da_similarity_mh_knn", "da_similarity_nw_knn", "da_dev_similarity_mh_knn", "da_dev_topk_rows_self", "da_dev_knn_edges_bytes",
               "da_dev_knn_edges"]
OK, EMPTY, BAD_K, BAD_NHASH, BAD_MATRIX, NO_DEVICE, UNSUPPORTED, BAD_ARG = 0, 1, 2, 3, 4, 8, 10, 11
SECOND = "a nearest neighbour needs a second sequence"


@pytest.fixture(scope="module")
def lib(built):
    from dynaalign_amd import _capi
    return _capi.load()


def test_header_library_and_signatures_agree_on_the_knn_symbols(lib):
    from dynaalign_amd import _capi
    declared = _capi.header_symbols()
    for name in KNN_SYMBOLS:
        assert name in declared, name
        assert name in _capi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert sorted(_capi.SIGNATURES) == declared
    assert lib.da_abi_version() == 2
    assert (_capi.DA_KNN_UNION, _capi.DA_KNN_MUTUAL) == (0, 1)
    header = open(_capi.HEADER_PATH).read()
    assert "#define DA_KNN_UNION 0" in header and "#define DA_KNN_MUTUAL 1" in header and "#define DA_ABI_VERSION 2" in header


def test_python_mirror_exports():
    import dynaalign_amd as da
    from dynaalign_amd import device, session
    for name in ("similarityMH_knn", "similarityNW_knn", "knn_dense", "knn_graph", "similarityMH_knn_edges", "similarityNW_knn_edges"):
        assert name in da.__all__ and callable(getattr(da, name)), name
    sig = inspect.signature(da.similarityMH_knn)
    assert list(sig.parameters) == ["sequences", "k", "n_hash", "top", "seed"]
    assert [sig.parameters[p].default for p in ("k", "n_hash", "top", "seed")] == [4, 50, 10, None]
    assert sig.parameters["seed"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(da.similarityNW_knn)
    assert list(sig.parameters) == ["sequences", "matrixName", "gapOpen", "gapExt", "top"]
    assert [sig.parameters[p].default for p in ("matrixName", "gapOpen", "gapExt", "top")] == ["BLOSUM62", 10, 4, 10]
    sig = inspect.signature(da.similarityMH_knn_edges)
    assert list(sig.parameters) == ["sequences", "k", "n_hash", "top", "mode", "seed"] and sig.parameters["mode"].default == "union"
    sig = inspect.signature(da.similarityNW_knn_edges)
    assert list(sig.parameters) == ["sequences", "matrixName", "gapOpen", "gapExt", "top", "mode"]
    sig = inspect.signature(da.knn_graph)
    assert list(sig.parameters) == ["idx", "val", "diag", "mode"] and sig.parameters["diag"].default is None
    sig = inspect.signature(device.topk_rows)
    assert list(sig.parameters) == ["keys", "top", "rank", "rank_bits", "self_col0", "want_self"]
    assert sig.parameters["self_col0"].default is None and sig.parameters["want_self"].default is False
    assert list(inspect.signature(device.similarity_mh_knn).parameters) == ["ds", "k", "n_hash", "seeds", "top"]
    sig = inspect.signature(device.knn_edges)
    assert list(sig.parameters) == ["idx", "key", "mode", "is_nw", "self_key", "self_code", "loops"]
    assert [sig.parameters[p].default for p in ("mode", "is_nw", "self_key", "self_code", "loops")] == ["union", False, None, 0, True]
    sig = inspect.signature(session.MinHashSession.knn)
    assert list(sig.parameters) == ["self", "top", "idx", "block_bytes"] and sig.parameters["top"].default == 10
    sig = inspect.signature(session.MinHashSession.knn_csr)
    assert list(sig.parameters) == ["self", "idx", "top", "mode"] and sig.parameters["mode"].default == "union"


def raw_mh(lib, seqs, k, nh, top, with_val=True, with_seeds=True):
    res, off = O.pack(seqs)
    seeds = np.zeros(max(nh, 1), np.uint32)
    cnt = max(len(seqs), 1) * max(top, 1)
    idx, val = np.full(cnt, -7, np.int32), np.full(cnt, -7.0)
    rc = lib.da_similarity_mh_knn(res.ctypes.data, off.ctypes.data, len(seqs), k, nh, seeds.ctypes.data if with_seeds else None, top,
                                  idx.ctypes.data, val.ctypes.data if with_val else None)
    return rc, lib.da_last_error().decode("latin-1") if rc else ""


def raw_nw(lib, seqs, top, matrix=b"BLOSUM62", with_diag=True):
    res, off = O.pack(seqs)
    cnt = max(len(seqs), 1) * max(top, 1)
    idx, val, diag = np.full(cnt, -7, np.int32), np.full(cnt, -7.0), np.full(max(len(seqs), 1), -7.0)
    rc = lib.da_similarity_nw_knn(res.ctypes.data, off.ctypes.data, len(seqs), matrix, 10, 4, top, idx.ctypes.data, val.ctypes.data,
                                  diag.ctypes.data if with_diag else None)
    return rc, lib.da_last_error().decode("latin-1") if rc else ""


def test_mh_validation_is_that_of_the_square_call_then_the_lists(lib, kats):
    import dynaalign_amd as da
    e = kats["mh_errors"]
    # n, k, n_hash in the reference's order and with its texts -- whatever top is, and before the second-sequence check
    for seqs, k, nh, code, msg in [([], 0, 0, EMPTY, e["empty"]), (["ACDE"], 0, 0, BAD_K, e["k"]), (["ACDE"], -1, 5, BAD_K, e["k"]),
                                   (["ACDE"], 4, 0, BAD_NHASH, e["n_hash"]), (["ACDE", "ACDF"], 4, -3, BAD_NHASH, e["n_hash"])]:
        for top in (0, 1, 5000):
            with pytest.raises(da.DynaAlignError) as ei:
                da.similarityMH_knn(seqs, k, nh, top)
            assert (ei.value.code, str(ei.value)) == (code, msg), (seqs, k, nh, top)
            with pytest.raises(da.DynaAlignError) as ej:
                da.similarityMH(seqs, k, nh)
            assert (ej.value.code, str(ej.value)) == (code, msg)
            assert raw_mh(lib, seqs, k, nh, top) == (code, msg)
    assert raw_mh(lib, ["ACDE", "ACDF"], 4, 8, 1, with_seeds=False)[0] == BAD_ARG            # NULL pointer
    # one sequence: no neighbour, whatever top
    for top in (0, 1, 2000):
        assert raw_mh(lib, ["ACDE"], 4, 8, top) == (BAD_ARG, SECOND)
    with pytest.raises(da.DynaAlignError) as ei:
        da.similarityMH_knn(["ACDE"], 4, 8)
    assert (ei.value.code, str(ei.value)) == (BAD_ARG, SECOND)
    # top: 1 .. n - 1, not clamped by the C ABI; beyond 1024 unsupported, with the text of the two-set form
    three = ["ACDEFGHIK", "ACDEFGHIR", "ACDEFGHIW"]
    for top in (0, -1, 3, 4):
        rc, msg = raw_mh(lib, three, 4, 8, top)
        assert rc == BAD_ARG and "top must be in 1 .. n - 1" in msg, (top, msg)
    big = ["ACDEFGHIK"] * 1027
    rc, msg = raw_mh(lib, big, 4, 8, 1025)
    assert rc == UNSUPPORTED and msg == "top-k per row keeps its candidates in a fixed LDS buffer: top <= 1024 (got 1025)"
    assert raw_mh(lib, big, 4, 8, 1027)[0] == BAD_ARG                                           # beyond n - 1 first
    # n_hash beyond the 16-bit counters: after top
    rc, msg = raw_mh(lib, three, 4, 70000, 2)
    assert rc == UNSUPPORTED and "65535" in msg
    assert raw_mh(lib, three, 4, 70000, 3)[0] == BAD_ARG
    assert raw_mh(lib, ["ACDE"], 4, 70000, 1) == (BAD_ARG, SECOND)


def test_device_forms_validate_before_they_look_at_a_pointer(lib):
    p = 4096
    for n, k, nh, code in [(0, 0, 0, EMPTY), (3, 0, 0, BAD_K), (3, 4, 0, BAD_NHASH)]:
        assert lib.da_dev_similarity_mh_knn(None, None, n, k, nh, None, 1, None, None, 1, None) == code
    assert lib.da_dev_similarity_mh_knn(None, None, 3, 4, 8, None, 1, None, None, 1, None) == BAD_ARG
    assert lib.da_dev_similarity_mh_knn(p, p, 1, 4, 8, p, 1, p, p, 1, None) == BAD_ARG
    assert lib.da_last_error().decode() == SECOND
    assert lib.da_dev_similarity_mh_knn(p, p, 3, 4, 8, p, 3, p, p, 3, None) == BAD_ARG          # top = n
    assert lib.da_dev_similarity_mh_knn(p, p, 3, 4, 8, p, 0, p, p, 3, None) == BAD_ARG
    assert lib.da_dev_similarity_mh_knn(p, p, 2000, 4, 8, p, 1025, p, p, 1025, None) == UNSUPPORTED
    assert lib.da_dev_similarity_mh_knn(p, p, 3, 4, 70000, p, 2, p, p, 2, None) == UNSUPPORTED
    assert lib.da_dev_similarity_mh_knn(p, p, 3, 4, 8, p, 2, p, p, 1, None) == BAD_ARG          # ld_out < top

    def tk(rows=4, n=100, ld=104, top=10, ld_out=10, keys=p, idx=p, key=p, bits=0, col0=0):
        return lib.da_dev_topk_rows_self(keys, rows, n, ld, None, bits, top, col0, idx, key, ld_out, None, None)
    assert tk(top=0) == BAD_ARG and tk(top=100) == BAD_ARG and tk(ld=99) == BAD_ARG and tk(ld_out=9) == BAD_ARG
    assert tk(top=100) == BAD_ARG and "1 .. n - 1" in lib.da_last_error().decode()            # top = n only through the plain form
    assert tk(keys=None) == BAD_ARG and tk(idx=None) == BAD_ARG and tk(key=None) == BAD_ARG and tk(bits=17) == BAD_ARG
    assert tk(n=2000, ld=2000, top=1025, ld_out=1025) == UNSUPPORTED
    assert tk(rows=0) == OK and tk(rows=-1) == BAD_ARG

    def ke(n=10, top=3, ld=3, mode=0, self_code=8, work=p * 256, idx=p, key=p, out=p):
        return lib.da_dev_knn_edges(idx, key, ld, n, top, mode, 0, None, self_code, 1, work, 1 << 20, out, out, out, out, None)
    assert ke(n=0) == EMPTY and ke(top=0) == BAD_ARG and ke(top=1025, ld=1025) == BAD_ARG and ke(ld=2) == BAD_ARG and ke(mode=2) == BAD_ARG
    assert ke(self_code=70000) == BAD_ARG and ke(idx=None) == BAD_ARG and ke(key=None) == BAD_ARG and ke(out=None) == BAD_ARG
    assert ke(work=None) == BAD_ARG and ke(work=p * 256 + 8) == BAD_ARG
    assert lib.da_dev_knn_edges_bytes(0, 10) > 0 and lib.da_dev_knn_edges_bytes(1000, 10) >= 2 * 1001 * 8


def test_nw_validation_follows_the_edge_list_call(lib, kats):
    import dynaalign_amd as da
    for seqs in (["AA", "AC"], [], ["AJ", "JJ"], ["AA"]):
        with pytest.raises(da.DynaAlignError) as ei:
            da.similarityNW_knn(seqs, "PAM250")
        assert (ei.value.code, str(ei.value)) == (BAD_MATRIX, kats["nw_bad_matrix"]["error"])
        assert raw_nw(lib, seqs, 1, b"PAM250")[0] == BAD_MATRIX
    for seqs in ([], ["AA"], ["AJ"]):                                            # a second sequence before anything about the residues
        assert raw_nw(lib, seqs, 1) == (BAD_ARG, SECOND)
    for top in (0, -1, 2, 3):
        rc, msg = raw_nw(lib, ["AA", "AJ"], top)
        assert rc == BAD_ARG and "top must be in 1 .. n - 1" in msg                # top before the residues, where thresh_p is checked
    rc, msg = raw_nw(lib, ["AA"] * 1027, 1025)
    assert rc == UNSUPPORTED and "1024" in msg
    # residue errors are those of da_similarity_nw_edges
    for seqs, code, msg in [(["JA", "AA"], O.ERR_BAD_RES1, "Invalid amino acid in sequence1: J"),
                            (["AJ", "AA"], O.ERR_BAD_RES2, "Invalid amino acid in sequence2: J"),
                            (["AA", "AJ"], O.ERR_BAD_RES2, "Invalid amino acid in sequence2: J"),
                            (["AA", "AC", "AU"], O.ERR_BAD_RES2, "Invalid amino acid in sequence2: U")]:
        assert raw_nw(lib, seqs, 1) == (code, msg), seqs
        thr, ne = np.zeros(1), np.zeros(1, np.int64)
        res, off = O.pack(seqs)
        assert lib.da_similarity_nw_edges(res.ctypes.data, off.ctypes.data, len(seqs), b"BLOSUM62", 10, 4, 0.5, thr.ctypes.data, ne.ctypes.data, 0,
                                          None, None, None) == code
        assert lib.da_last_error().decode("latin-1") == msg
    # an empty sequence is refused, and so is one beyond the 8-bit alignment length; both after the residues
    rc, msg = raw_nw(lib, ["AA", "", "AC"], 1)
    assert rc == UNSUPPORTED and "sequence 2 is empty" in msg and "NaN" in msg
    rc, msg = raw_nw(lib, ["A" * 128, "AA"], 1)
    assert rc == UNSUPPORTED and "127" in msg
    assert raw_nw(lib, ["A" * 128, "AJ"], 1)[0] == O.ERR_BAD_RES2


def test_python_mirror_clamps_top_and_valid_input_fails_loudly_without_a_device(lib):
    import dynaalign_amd as da
    seqs = ["ACDEFG", "ACDEFH", "ACDEFK"]
    calls = (lambda: da.similarityMH_knn(seqs, 4, 8, 9, seed=1), lambda: da.similarityNW_knn(seqs, top=9))
    for call in calls:
        if lib.da_device_count() > 0:
            idx, val = call()
            assert idx.shape == (3, 2) and val.shape == (3, 2) and idx.dtype == np.int32 and val.dtype == np.float64
        else:
            with pytest.raises(da.DynaAlignError) as ei:
                call()
            assert ei.value.code == NO_DEVICE and "no CPU fallback" in str(ei.value)
    want = OK if lib.da_device_count() > 0 else NO_DEVICE
    assert raw_mh(lib, seqs, 4, 8, 2)[0] == want and raw_mh(lib, seqs, 4, 8, 2, with_val=False)[0] == want
    assert raw_nw(lib, seqs, 2)[0] == want and raw_nw(lib, seqs, 2, with_diag=False)[0] == want
