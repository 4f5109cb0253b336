"""CPU tests of the NW identity on MinHash LSH candidates: the numpy definitions (nw_lsh_edges_dense, nw_lsh_cross_edges_dense) against a
slow Python model built on the LSH model of test_lsh_cpu.py and the oracle's pair value, exports, the C ABI's symbols, the size of the
rescore workspace, and the validation order and texts of da_similarity_nw_lsh_edges_begin / da_similarity_nw_lsh_cross_edges_begin --
every error arrives before a device is needed.  Nothing here computes on a device unless one is present (the accepted cases)."""
import ctypes
import inspect

import numpy as np
import pytest

import oracle_lib as O
from test_lsh_cpu import model
from test_lsh_cross_cpu import cross_model

NW_LSH_SYMBOLS = ["da_similarity_nw_lsh_edges_begin", "da_similarity_nw_lsh_cross_edges_begin", "da_nw_lsh_last_route", "da_dev_nw_rescore_pairs",
                  "da_dev_nw_rescore_workspace_bytes", "da_dev_lsh_nw_edges", "da_dev_lsh_cross_nw_edges"]
OK, EMPTY, BAD_K, BAD_NHASH, BAD_MATRIX, BAD_RES1, BAD_RES2, NO_DEVICE, UNSUPPORTED, BAD_ARG = 0, 1, 2, 3, 4, 5, 6, 8, 10, 11
AA20 = "ACDEFGHIKLMNPQRSTVWY"


def nw_value_of(x, y, matrix="BLOSUM62", go=10, ge=4):
    """-> nw_value(i, j): the oracle's matches / length of x[i] as sequence1 against y[j] as sequence2, one Python divide"""
    def value(i, j):
        rc, mt, ln, _, _ = O.nw_pair(x[i], y[j], matrix, go, ge)
        assert rc == 0 and ln > 0
        return mt / ln
    return value


def nw_model(cand_i, cand_j, value, threshold):
    """the candidates one by one -> dict i, j, w (sorted as the candidates are) and every candidate's value"""
    out = {"i": [], "j": [], "w": [], "all": {}}
    for i, j in zip(cand_i, cand_j):
        w = value(i, j)
        out["all"][(i, j)] = w
        if w >= threshold and w > 0:
            out["i"].append(i); out["j"].append(j); out["w"].append(w)
    return out


def same_edges(got, want):
    i, j, w = got
    assert np.asarray(i).dtype == np.int32 and np.asarray(j).dtype == np.int32 and np.asarray(w).dtype == np.float64
    assert np.asarray(i).tolist() == want["i"] and np.asarray(j).tolist() == want["j"]
    assert np.array_equal(np.asarray(w).view(np.uint64), np.array(want["w"], np.float64).view(np.uint64))


@pytest.fixture(scope="module")
def strings():
    from test_gpu_jaccard import family
    return family(3, 5, 20, 40) + ["A", "AC", AA20, AA20[::-1], "XXXXXXXXXX"]


@pytest.mark.parametrize("bands,rows,mh_thr,thr,go,ge", [(12, 4, 0.0, 0.5, 10, 4), (12, 4, 0.5, 0.0, 10, 4), (48, 1, 0.0, 1.0, 10, 4),
                                                       (12, 4, 0.0, 0.5, 0, 0)])
def test_dense_definition_against_the_model(built, strings, bands, rows, mh_thr, thr, go, ge):
    import dynaalign_amd as da
    sig = O.signatures(strings, 4, 48, O.seeds(12345, 48))
    cand = model(sig, bands, rows, mh_thr)
    value = nw_value_of(strings, strings, "BLOSUM62", go, ge)
    want = nw_model(cand["i"], cand["j"], value, thr)
    assert len(cand["i"]) > len(strings) and 0 < len(want["i"]) <= len(cand["i"])
    assert thr == 0.0 or len(want["i"]) < len(cand["i"])
    if go == 0:                                   # the diagonal is scored: at free gaps X against X (score -1) is all gaps but one step: 1 / 19
        x = strings.index("XXXXXXXXXX")
        assert want["all"][(x, x)] < 0.5 and (x, x) not in set(zip(want["i"], want["j"]))
    same_edges(da.nw_lsh_edges_dense(sig, bands, rows, mh_thr, value, thr), want)


def test_cross_definition_against_the_model(built, strings):
    import dynaalign_amd as da
    x, y = strings[:15] + ["ACDEFGHIKL"], strings[10:]
    sv = O.seeds(7, 40)
    sx, sy = O.signatures(x, 4, 40, sv), O.signatures(y, 4, 40, sv)
    cand = cross_model(sx, sy, 10, 4, 0.3)
    value = nw_value_of(x, y)
    want = nw_model(cand["i"], cand["j"], value, 0.9)
    assert 0 < len(want["i"]) < len(cand["i"])
    same_edges(da.nw_lsh_cross_edges_dense(sx, sy, 10, 4, 0.3, value, 0.9), want)


def test_exports_and_parameter_lists():
    import dynaalign_amd as da
    from dynaalign_amd import device
    for name in ("similarityNW_lsh_edges", "similarityNW_lsh_cross_edges", "nw_lsh_edges_dense", "nw_lsh_cross_edges_dense", "nw_lsh_last_route"):
        assert name in da.__all__ and callable(getattr(da, name)), name
    sig = inspect.signature(da.similarityNW_lsh_edges)
    assert list(sig.parameters) == ["sequences", "k", "n_hash", "bands", "rows", "threshold", "mh_threshold", "matrixName", "gapOpen", "gapExt", "seed",
                                    "max_candidates"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [4, 50, 10, 5, 0.5, 0.0, "BLOSUM62", 10, 4, None, 1 << 32]
    assert all(sig.parameters[p].kind is inspect.Parameter.KEYWORD_ONLY for p in ("mh_threshold", "matrixName", "gapOpen", "gapExt", "seed", "max_candidates"))
    cross = inspect.signature(da.similarityNW_lsh_cross_edges)
    assert list(cross.parameters) == ["x", "y"] + list(sig.parameters)[1:]
    assert list(inspect.signature(da.nw_lsh_edges_dense).parameters) == ["sig", "bands", "rows", "mh_threshold", "nw_value", "threshold"]
    assert list(inspect.signature(da.nw_lsh_cross_edges_dense).parameters) == ["sig_x", "sig_y", "bands", "rows", "mh_threshold", "nw_value", "threshold"]
    assert list(inspect.signature(device.nw_rescore_pairs).parameters)[:4] == ["dx", "dy", "i", "j"]
    assert list(inspect.signature(device.lsh_nw_edges).parameters)[:2] == ["sig", "ds"]


@pytest.fixture(scope="module")
def lib(built):
    from dynaalign_amd import _capi
    return _capi.load()


def test_header_library_and_signatures_agree(lib):
    from dynaalign_amd import _capi
    declared = _capi.header_symbols()
    for name in NW_LSH_SYMBOLS:
        assert name in declared, name
        assert name in _capi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert sorted(_capi.SIGNATURES) == declared
    assert lib.da_abi_version() == 2


def test_rescore_workspace_bytes(lib):
    size = lib.da_dev_nw_rescore_workspace_bytes
    for pairs in (0, -1, -(1 << 40)):
        assert size(pairs, 1024, 0) == 0 and size(pairs, 1024, 1) == 0
    counts = [1, 2, 63, 64, 65, 128, 4097, 100000, 1 << 18, (1 << 18) + 1, 1 << 20, 1 << 24, 50000000]
    for minimal in (0, 1):
        sizes = [size(p, 1024, minimal) for p in counts]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
        assert sizes[0] > 0
    for p in counts:
        assert size(p, 1024, 1) <= size(p, 1024, 0)
        assert size(p, 1024, 1) >= 5 * 4 * p + p                # three index lists and two result lists of int32, a class byte
        assert size(p, 20, 0) == size(p, 1024, 0)                # the lengths do not enter
    assert size(64, 1024, 1) == size(64, 1024, 0)                # one wavefront of pairs is the minimum in flight


def raw(lib, seqs, k=4, nh=8, bands=2, rows=4, mh_thr=0.0, maxc=1 << 32, matrix=b"BLOSUM62", thr=0.5, *, seeds=True, offsets=True, off=None,
        handle=True, count=True, y=None, y_off=None):
    """da_similarity_nw_lsh_edges_begin (y None) / da_similarity_nw_lsh_cross_edges_begin through ctypes -> (status, text)"""
    res, o = O.pack(seqs)
    if off is not None:
        o = np.asarray(off, np.int64)
    sv = np.zeros(max(nh, 1), np.uint32)
    h = ctypes.c_void_p()
    cnt = np.zeros(1, np.int64)
    tail = (k, nh, sv.ctypes.data if seeds else None, bands, rows, mh_thr, maxc, matrix, 10, 4, thr, ctypes.addressof(h) if handle else None,
            cnt.ctypes.data if count else None)
    if y is None:
        rc = lib.da_similarity_nw_lsh_edges_begin(res.ctypes.data, o.ctypes.data if offsets else None, len(seqs), *tail)
    else:
        yres, yo = O.pack(y)
        if y_off is not None:
            yo = np.asarray(y_off, np.int64)
        rc = lib.da_similarity_nw_lsh_cross_edges_begin(res.ctypes.data, o.ctypes.data if offsets else None, len(seqs), yres.ctypes.data, yo.ctypes.data,
                                                        len(y), *tail)
    if rc == OK:
        assert h.value
        lib.da_edges_free(h)
    else:
        assert not h.value
    return rc, lib.da_last_error().decode("latin-1") if rc else ""


def test_validation_order_and_texts(lib, kats):
    import dynaalign_amd as da
    e = kats["mh_errors"]
    two = ["ACDEFGHIK", "ACDEFGHIR"]
    nan = float("nan")
    bad_matrix = (BAD_MATRIX, "Invalid substitution matrix name: PAM250")
    # 0: the matrix name, before everything -- an empty input, NULL pointers
    assert raw(lib, [], 0, 0, 0, 0, nan, -1, b"PAM250", nan, seeds=False, offsets=False, handle=False) == bad_matrix
    # 1-3: n, k, n_hash with the texts of similarityMH, each before everything behind it
    assert raw(lib, [], 0, 0, 0, 0, nan, -1, thr=nan, seeds=False, offsets=False, handle=False) == (EMPTY, e["empty"])
    assert raw(lib, two, 0, 0, 0, 0, nan, -1, thr=nan, seeds=False, offsets=False) == (BAD_K, e["k"])
    assert raw(lib, two, 4, 0, 0, 0, nan, -1, thr=nan, seeds=False, offsets=False) == (BAD_NHASH, e["n_hash"])
    # 4: NULL pointers, before the offsets are looked at
    for kw in ({"seeds": False}, {"handle": False}, {"count": False}):
        assert raw(lib, two, 4, 8, 0, 0, nan, -1, thr=nan, off=[3, 2, 1], **kw) == (BAD_ARG, "NULL pointer"), kw
    # 5: offsets, before bands / rows
    assert raw(lib, two, 4, 8, 0, 0, nan, -1, thr=nan, offsets=False) == (BAD_ARG, "offsets is NULL")
    assert raw(lib, two, 4, 8, 0, 0, nan, -1, thr=nan, off=[0, 9, 5]) == (BAD_ARG, "offsets must be non-decreasing (sequence 1)")
    assert raw(lib, two, 4, 8, 0, 0, nan, -1, thr=nan, off=[1, 9, 18]) == (BAD_ARG, "offsets[0] must be 0")
    # 6: bands, rows, their product, the cap, the 16-bit limit of n_hash -- the texts of the MinHash call, all before the residues are read
    bad = ["ACDEFGHIK", "ACDEFGHIJ"]
    assert raw(lib, bad, 4, 8, 0, 0, nan, -1, thr=nan) == (BAD_ARG, "bands must be >= 1 (got 0)")
    assert raw(lib, bad, 4, 8, 2, 0, nan, -1, thr=nan) == (BAD_ARG, "rows must be >= 1 (got 0)")
    assert raw(lib, bad, 4, 8, 3, 4, nan, -1, thr=nan) == (BAD_ARG, "bands * rows = 12 exceeds n_hash = 8")
    assert raw(lib, bad, 4, 8, 2, 4, nan, -1, thr=nan) == (BAD_ARG, "max_candidates must be >= 0 (got -1)")
    assert raw(lib, bad, 4, 65536, 2, 4, nan, thr=nan) == (UNSUPPORTED, "the LSH edge list counts in 16 bits: n_hash <= 65535 (got 65536)")
    # 7: the NW checks: invalid residues, an empty sequence, one over 1024 residues -- before the thresholds
    assert raw(lib, bad, mh_thr=nan, thr=nan) == (BAD_RES2, "Invalid amino acid in sequence2: J")
    assert raw(lib, ["JCDEFGHIK", "ACDEFGHIK"], mh_thr=nan, thr=nan) == (BAD_RES1, "Invalid amino acid in sequence1: J")
    rc, text = raw(lib, ["ACDEFGHIK", "", "A" * 1025], mh_thr=nan, thr=nan)
    assert rc == UNSUPPORTED and text.startswith("sequence 2 is empty")
    rc, text = raw(lib, ["ACDEFGHIK", "A" * 1025], mh_thr=nan, thr=nan)
    assert rc == UNSUPPORTED and text == "the alignment kernels take sequences up to 1024 residues (sequence 2: 1025)"
    # 8: threshold, then mh_threshold
    for v in (nan, -0.001, 1.001, float("inf")):
        assert raw(lib, two, mh_thr=nan, thr=v) == (BAD_ARG, "threshold must be in [0, 1]"), v
        assert raw(lib, two, mh_thr=v, thr=0.5) == (BAD_ARG, "mh_threshold must be in [0, 1]"), v
    # accepted (a device is needed only now): 1024 residues, the thresholds 0 and 1, n = 1
    want = OK if lib.da_device_count() > 0 else NO_DEVICE
    assert raw(lib, two)[0] == want
    assert raw(lib, ["ACDEFGHIK", "A" * 1024], mh_thr=1.0, thr=0.0)[0] == want
    assert raw(lib, ["ACDEFGHIK"], mh_thr=0.0, thr=1.0, maxc=0)[0] == want
    # the Python entry point passes the library's errors on
    for args, kw, code, msg in [((two,), {"matrixName": "PAM250"}, *bad_matrix), (([],), {}, EMPTY, e["empty"]),
                                ((two, 4, 8, 3, 3), {}, BAD_ARG, "bands * rows = 9 exceeds n_hash = 8"),
                                ((bad, 4, 8, 2, 4), {}, BAD_RES2, "Invalid amino acid in sequence2: J"),
                                ((two, 4, 8, 2, 4, 1.5), {}, BAD_ARG, "threshold must be in [0, 1]"),
                                ((two, 4, 8, 2, 4, 0.5), {"mh_threshold": -1.0}, BAD_ARG, "mh_threshold must be in [0, 1]")]:
        with pytest.raises(da.DynaAlignError) as ei:
            da.similarityNW_lsh_edges(*args, seed=1, **kw)
        assert (ei.value.code, str(ei.value)) == (code, msg), args


def test_cross_validation_order_and_texts(lib, kats):
    import dynaalign_amd as da
    e = kats["mh_errors"]
    x, y = ["ACDEFGHIK", "ACDEFGHIR"], ["ACDEFGHIK", "WCDEFGHIR", "ACDEF"]
    nan = float("nan")
    bad_matrix = (BAD_MATRIX, "Invalid substitution matrix name: PAM250")
    assert raw(lib, [], 0, 0, 0, 0, nan, -1, b"PAM250", nan, y=[], seeds=False, offsets=False, handle=False) == bad_matrix
    # x empty, y empty, k, n_hash
    assert raw(lib, [], 0, 0, 0, 0, nan, -1, thr=nan, y=y, seeds=False) == (EMPTY, e["empty"])
    assert raw(lib, x, 0, 0, 0, 0, nan, -1, thr=nan, y=[], seeds=False) == (EMPTY, e["empty"])
    assert raw(lib, x, 0, 0, 0, 0, nan, -1, thr=nan, y=y, seeds=False) == (BAD_K, e["k"])
    assert raw(lib, x, 4, 0, 0, 0, nan, -1, thr=nan, y=y, seeds=False) == (BAD_NHASH, e["n_hash"])
    # NULL pointers, the offsets of x, the offsets of y
    for kw in ({"seeds": False}, {"handle": False}, {"count": False}):
        assert raw(lib, x, 4, 8, 0, 0, nan, -1, thr=nan, y=y, off=[3, 2, 1], **kw) == (BAD_ARG, "NULL pointer"), kw
    assert raw(lib, x, 4, 8, 0, 0, nan, -1, thr=nan, y=y, off=[0, 9, 5], y_off=[1, 2, 3, 4]) == (BAD_ARG, "offsets must be non-decreasing (sequence 1)")
    assert raw(lib, x, 4, 8, 0, 0, nan, -1, thr=nan, y=y, y_off=[1, 9, 18, 23]) == (BAD_ARG, "offsets[0] must be 0")
    # the banding and the cap, before the residues
    yb = ["ACDEFGHIK", "ACDEFGHIJ"]
    assert raw(lib, x, 4, 8, 0, 0, nan, -1, thr=nan, y=yb) == (BAD_ARG, "bands must be >= 1 (got 0)")
    assert raw(lib, x, 4, 8, 2, 0, nan, -1, thr=nan, y=yb) == (BAD_ARG, "rows must be >= 1 (got 0)")
    assert raw(lib, x, 4, 8, 3, 4, nan, -1, thr=nan, y=yb) == (BAD_ARG, "bands * rows = 12 exceeds n_hash = 8")
    assert raw(lib, x, 4, 8, 2, 4, nan, -1, thr=nan, y=yb) == (BAD_ARG, "max_candidates must be >= 0 (got -1)")
    assert raw(lib, x, 4, 65536, 2, 4, nan, thr=nan, y=yb) == (UNSUPPORTED, "the LSH edge list counts in 16 bits: n_hash <= 65535 (got 65536)")
    # the NW checks: residues in the order of similarityNW_cross, an empty sequence of either set, one over 1024 residues
    assert raw(lib, x, mh_thr=nan, thr=nan, y=yb) == (BAD_RES2, "Invalid amino acid in sequence2: J")
    assert raw(lib, ["JCDEFGHIK"], mh_thr=nan, thr=nan, y=yb) == (BAD_RES1, "Invalid amino acid in sequence1: J")
    rc, text = raw(lib, ["ACDEFGHIK", ""], mh_thr=nan, thr=nan, y=["A" * 1025])
    assert rc == UNSUPPORTED and text.startswith("sequence 2 of x is empty")
    rc, text = raw(lib, x, mh_thr=nan, thr=nan, y=["ACD", "", "A" * 1025])
    assert rc == UNSUPPORTED and text.startswith("sequence 2 of y is empty")
    rc, text = raw(lib, x, mh_thr=nan, thr=nan, y=["ACD", "A" * 1025])
    assert rc == UNSUPPORTED and text == "the alignment kernels take sequences up to 1024 residues (sequence 2 of y: 1025)"
    # threshold, then mh_threshold; then the device
    for v in (nan, -0.001, 1.001):
        assert raw(lib, x, mh_thr=nan, thr=v, y=y) == (BAD_ARG, "threshold must be in [0, 1]"), v
        assert raw(lib, x, mh_thr=v, thr=0.5, y=y) == (BAD_ARG, "mh_threshold must be in [0, 1]"), v
    want = OK if lib.da_device_count() > 0 else NO_DEVICE
    assert raw(lib, x, y=y)[0] == want
    assert raw(lib, x, mh_thr=1.0, thr=0.0, y=["A" * 1024])[0] == want
    with pytest.raises(da.DynaAlignError) as ei:
        da.similarityNW_lsh_cross_edges(x, y, 4, 8, 2, 4, 2.0, seed=1)
    assert (ei.value.code, str(ei.value)) == (BAD_ARG, "threshold must be in [0, 1]")


def test_last_route_needs_no_device_and_skips_null(lib):
    import dynaalign_amd as da
    v = np.full(7, -1, np.int64)
    assert lib.da_nw_lsh_last_route(v.ctypes.data, None, None, v[3:].ctypes.data, None, None, v[6:].ctypes.data) == OK
    assert v[0] >= 0 and v[1] == -1 and v[2] == -1 and v[3] >= 0 and v[4] == -1 and v[5] == -1 and v[6] >= 0
    assert sorted(da.nw_lsh_last_route()) == ["aligned_pairs", "buckets", "edges", "incidences", "long_pairs", "short_pairs", "verified_pairs"]
