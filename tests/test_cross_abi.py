"""CPU tests of the two-set boundary (similarityMH_cross / similarityNW_cross and the device-side rectangle calls): symbols, validation
order and texts, the NW residue errors of the reference's lazy fill, and the refusal to compute without a GPU.  No compute calls here."""
import numpy as np
import pytest

import oracle_lib as O


@pytest.fixture(scope="module")
def lib(built):
    from dynaalign_amd import _capi
    return _capi.load()


CROSS_SYMBOLS = ["da_similarity_mh_cross", "da_similarity_nw_cross", "da_dev_mh_compare_rect", "da_dev_nw_rect",
                 "da_dev_similarity_mh_cross", "da_mh_cross_last_route"]


def test_header_library_and_signatures_agree_on_the_cross_symbols(lib):
    from dynaalign_amd import _capi
    declared = _capi.header_symbols()
    for name in CROSS_SYMBOLS:
        assert name in declared, name
        assert name in _capi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert sorted(_capi.SIGNATURES) == declared
    assert lib.da_abi_version() == 2


def test_python_mirror_exports():
    import dynaalign_amd as da
    from dynaalign_amd import device, session
    assert callable(da.similarityMH_cross) and callable(da.similarityNW_cross)
    for name in ("mh_compare_rect", "nw_rect", "similarity_mh_cross", "mh_cross_last_route"):
        assert callable(getattr(device, name)), name
    assert callable(session.MinHashSession.cross)
    m = da.SimilarityMatrix(np.zeros((2, 3)))
    assert m.dimnames == [["1", "2"], ["1", "2", "3"]]
    assert da.SimilarityMatrix(np.zeros((2, 2))).dimnames == [["1", "2"], ["1", "2"]]


def test_mh_validation_order_and_texts(lib, kats):
    import dynaalign_amd as da
    e = kats["mh_errors"]
    # x empty, then y empty, then k, then n_hash
    for x, y, k, nh, code, msg in [([], [], 0, 0, 1, e["empty"]), ([], ["ACDE"], 0, 0, 1, e["empty"]), (["ACDE"], [], 0, 0, 1, e["empty"]),
                                   (["ACDE"], ["ACDE"], 0, 0, 2, e["k"]), (["ACDE"], ["ACDE"], -1, 5, 2, e["k"]),
                                   (["ACDE"], ["ACDE"], 4, 0, 3, e["n_hash"]), (["ACDE"], ["ACDE"], 4, -3, 3, e["n_hash"])]:
        with pytest.raises(da.DynaAlignError) as ei:
            da.similarityMH_cross(x, y, k, nh)
        assert (ei.value.code, str(ei.value)) == (code, msg), (x, y, k, nh)
    # the device form validates alike, before it looks at a pointer
    for m, n, k, nh, code in [(0, 0, 0, 0, 1), (0, 3, 4, 8, 1), (3, 0, 4, 8, 1), (3, 3, 0, 0, 2), (3, 3, 4, 0, 3)]:
        assert lib.da_dev_similarity_mh_cross(None, None, m, 0, None, None, n, 0, k, nh, None, None, n, None) == code
    assert lib.da_dev_similarity_mh_cross(None, None, 3, 0, None, None, 3, 0, 4, 8, None, None, 3, None) == 11
    # n_hash beyond the 16-bit counters is refused loudly (valid pointers: the check comes after the NULL test)
    res, off = O.pack(["ACDE"])
    seeds, out = np.zeros(70000, np.uint32), np.zeros(1)
    assert lib.da_similarity_mh_cross(res.ctypes.data, off.ctypes.data, 1, res.ctypes.data, off.ctypes.data, 1, 4, 70000, seeds.ctypes.data,
                                      out.ctypes.data, 0) == 10


def test_nw_matrix_name_first_and_empty_sides(lib, kats):
    import dynaalign_amd as da
    for x, y in [(["AA"], ["AA"]), ([], ["AA"]), (["AA"], []), (["AJ"], ["JJ"])]:
        with pytest.raises(da.DynaAlignError) as ei:
            da.similarityNW_cross(x, y, "PAM250")
        assert (ei.value.code, str(ei.value)) == (4, kats["nw_bad_matrix"]["error"])
    r = da.similarityNW_cross([], ["AA"])
    assert r.shape == (0, 1) and r.dimnames == [[], ["1"]]
    assert da.similarityNW_cross(["AA"], []).shape == (1, 0)
    assert da.similarityNW_cross([], []).shape == (0, 0)
    assert da.similarityNW_cross([], ["J"]).shape == (0, 1)          # nothing is visited, nothing is raised


def expected_nw_error(x, y):
    """first non-zero rc of the oracle's calc over the pairs, i outer over x, j inner over y"""
    for a in x:
        for b in y:
            rc, _, _, _, bad = O.nw_pair(a, b)
            if rc:
                return rc, "Invalid amino acid in sequence%d: %s" % (1 if rc == O.ERR_BAD_RES1 else 2, bad)
    return 0, ""


def raw_nw_cross(lib, x, y, column_major):
    xr, xo = O.pack(x)
    yr, yo = O.pack(y)
    out = np.zeros(max(len(x) * len(y), 1))
    rc = lib.da_similarity_nw_cross(xr.ctypes.data, xo.ctypes.data, len(x), yr.ctypes.data, yo.ctypes.data, len(y), b"BLOSUM62", 10, 4,
                                    out.ctypes.data, column_major)
    return rc, lib.da_last_error().decode("latin-1") if rc else ""


@pytest.mark.parametrize("x,y", [
    (["AJ"], ["AA"]), (["AA"], ["AJ"]), (["", "JA"], ["AA"]), (["AA"], ["", "J"]), (["A"], ["J", "AA"]), (["J"], ["", "AA"]),
    (["JA"], ["UA"]), (["AJ"], ["UA"]), (["AA", "AJ"], ["AA", "AU"]), (["", ""], ["J"]), (["A A"], ["AA"]), (["AA"], ["a"]),
    (["AJU"], ["", "O"]), (["A", "J"], ["", ""]),
])
def test_nw_residue_errors_match_the_lazy_reference_order(lib, x, y):
    rc, msg = expected_nw_error(x, y)
    if (x, y) == (["J"], ["", "AA"]):
        assert (rc, msg) == (O.ERR_BAD_RES1, "Invalid amino acid in sequence1: J")   # raised against the empty y[0]
    for cm in (0, 1):
        got = raw_nw_cross(lib, x, y, cm)
        if rc:
            assert got == (rc, msg), (x, y, cm)
        else:
            assert got[0] in (0, 8), (x, y, cm)      # valid input: computed, or refused for want of a device


def test_nw_errors_fuzz(lib):
    rng = np.random.RandomState(11)
    alpha = "ARNDCQEGHILKMFPSTWYVBZX*" * 3 + "JUO"
    seen = set()

    def draw():
        return ["".join(alpha[i] for i in rng.randint(0, len(alpha), rng.randint(0, 6))) for _ in range(rng.randint(1, 5))]
    for _ in range(200):
        x, y = draw(), draw()
        rc, msg = expected_nw_error(x, y)
        if rc == 0:
            continue
        seen.add(rc)
        for cm in (0, 1):
            assert raw_nw_cross(lib, x, y, cm) == (rc, msg), (x, y, cm)
    assert seen == {O.ERR_BAD_RES1, O.ERR_BAD_RES2}


def test_valid_input_fails_loudly_without_a_device(lib):
    import dynaalign_amd as da
    if lib.da_device_count() > 0:       # with a device, valid input computes: the values are the GPU tests' business, the shapes are checked here
        assert da.similarityMH_cross(["ACDEFG", "ACDEFH"], ["ACDEFG"], 4, 8, seed=1).shape == (2, 1)
        assert da.similarityNW_cross(["ACDEFG", "ACDEFH"], ["ACDEFG"]).shape == (2, 1)
        for cm in (0, 1):
            assert raw_nw_cross(lib, ["ACD"], ["AC", ""], cm)[0] == 0
        return
    with pytest.raises(da.DynaAlignError) as ei:
        da.similarityMH_cross(["ACDEFG", "ACDEFH"], ["ACDEFG"], 4, 8, seed=1)
    assert ei.value.code == 8 and "no CPU fallback" in str(ei.value)
    with pytest.raises(da.DynaAlignError) as ei:
        da.similarityNW_cross(["ACDEFG", "ACDEFH"], ["ACDEFG"])
    assert ei.value.code == 8
    for cm in (0, 1):
        assert raw_nw_cross(lib, ["ACD"], ["AC", ""], cm)[0] == 8


def test_rect_calls_refuse_bad_arguments(lib):
    BAD = 11
    p = 4096                                   # any non-NULL, 16-byte aligned value: the checks below never dereference it
    n, nh = 300, 50

    def mh(rb=0, re_=100, cb=128, ce=300, kind=0, ld=172, planes=p, out=p, bits=12):
        return lib.da_dev_mh_compare_rect(planes, bits, n, nh, rb, re_, cb, ce, kind, out, ld, None)
    assert mh(cb=-1) == BAD and mh(ce=301) == BAD and mh(cb=200, ce=100) == BAD      # column range outside [0, n] / reversed
    assert mh(rb=-1) == BAD and mh(re_=301) == BAD
    assert mh(ld=171) == BAD                                                          # ld < columns
    assert mh(planes=None) == BAD and mh(out=None) == BAD
    assert mh(kind=2) == BAD and mh(bits=13) == BAD and mh(planes=p + 4) == BAD

    def nw(rb=0, re_=100, cb=128, ce=300, kind=0, ld=172, codes=p, off=p, out=p):
        return lib.da_dev_nw_rect(codes, off, n, 20, 0, 10, 4, rb, re_, cb, ce, kind, out, ld, None)
    assert nw(cb=-1) == BAD and nw(ce=301) == BAD and nw(cb=200, ce=100) == BAD
    assert nw(rb=-1) == BAD and nw(re_=301) == BAD
    assert nw(ld=171) == BAD
    assert nw(codes=None) == BAD and nw(off=None) == BAD and nw(out=None) == BAD
    assert nw(kind=3) == BAD
