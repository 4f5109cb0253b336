"""CPU tests of the NW-ranked nearest-neighbour lists on MinHash LSH candidates: the numpy definitions (nw_lsh_knn_dense,
nw_lsh_cross_topk_dense) against a brute-force per-row Python sort over the LSH model of test_lsh_cpu.py and the oracle's pair value,
exports, the C ABI's symbols and prototypes, and the validation order and texts of da_similarity_nw_lsh_knn /
da_similarity_nw_lsh_cross_topk -- every error arrives before a device is needed.  Nothing here computes on a device unless one is
present (the accepted cases)."""
import inspect

import numpy as np
import pytest

import oracle_lib as O
from test_lsh_cpu import model
from test_lsh_cross_cpu import cross_model
from test_nw_lsh_cpu import AA20, nw_value_of

SYMBOLS = ["da_similarity_nw_lsh_knn", "da_similarity_nw_lsh_cross_topk", "da_dev_lsh_nw_knn", "da_dev_lsh_cross_nw_topk", "da_dev_nw_knn_select",
           "da_dev_nw_rank_keys"]
OK, EMPTY, BAD_K, BAD_NHASH, BAD_MATRIX, BAD_RES1, BAD_RES2, NO_DEVICE, UNSUPPORTED, BAD_ARG = 0, 1, 2, 3, 4, 5, 6, 8, 10, 11


def rows_model(n_rows, cand_i, cand_j, value, top, threshold, one_set):
    """Brute force, row by row.  one_set: the candidates (i, i) give diag, every i < j is scored once -- the smaller position as sequence1
    -- and listed in both rows; otherwise the rows of x only.  A row keeps w >= threshold and w > 0, sorted by (-w, column), cut at top,
    padded -1 / 0.0.  -> (idx lists, val lists, diag list, degrees before the cut, {pair: w})"""
    rows = [[] for _ in range(n_rows)]
    diag = [0.0] * n_rows
    scored = {}
    for i, j in zip(cand_i, cand_j):
        if one_set:
            assert i <= j
        w = value(i, j)
        scored[(i, j)] = w
        if one_set and i == j:
            diag[i] = w
            continue
        if w >= threshold and w > 0:
            rows[i].append((-w, j))
            if one_set:
                rows[j].append((-w, i))
    idx, val = [], []
    for r in rows:
        r.sort()
        first = r[:top]
        idx.append([c for _, c in first] + [-1] * (top - len(first)))
        val.append([-w for w, _ in first] + [0.0] * (top - len(first)))
    return idx, val, diag, [len(r) for r in rows], scored


def same_lists(got, idx, val, diag=None):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64
    assert got[0].tolist() == idx
    assert np.array_equal(got[1].view(np.uint64), np.array(val, np.float64).reshape(got[1].shape).view(np.uint64))
    if diag is not None:
        assert np.array_equal(np.asarray(got[2], np.float64).view(np.uint64), np.array(diag, np.float64).view(np.uint64))


@pytest.fixture(scope="module")
def strings():
    from test_gpu_jaccard import family
    rng = np.random.RandomState(4)
    out = family(3, 5, 20, 36)
    for _ in range(4):                              # q, q + tail (10 / 20) and q[:5] (5 / 10): one double from two (matches, length)
        q = "".join(AA20[t] for t in rng.randint(0, 20, 10))
        out += [q, q + "".join(AA20[t] for t in rng.randint(0, 20, 10)), q[:5]]
    out = list(dict.fromkeys(out + ["X" * 10, "X" * 20, "X" * 9 + "A"]))
    assert 40 <= len(out) <= 60
    return out


@pytest.mark.parametrize("bands,rows,mh_thr,thr,go,ge", [(12, 4, 0.0, 0.0, 10, 4), (12, 4, 0.0, 0.5, 10, 4), (48, 1, 0.0, 0.0, 10, 4),
                                                       (48, 1, 0.25, 0.5, 10, 4), (48, 1, 0.0, 0.0, 0, 0)])
def test_dense_definition_against_the_row_sort(built, strings, bands, rows, mh_thr, thr, go, ge):
    import dynaalign_amd as da
    sig = O.signatures(strings, 4, 48, O.seeds(12345, 48))
    cand = model(sig, bands, rows, mh_thr)
    value = nw_value_of(strings, strings, "BLOSUM62", go, ge)
    n = len(strings)
    full = rows_model(n, cand["i"], cand["j"], value, 1024, thr, True)
    degs = full[3]
    assert max(degs) > 1 and (rows == 1 or min(degs) == 0)   # top = 1 cuts a row; with 12 x 4 some row is all padding
    if go == 0:                                     # w > 0: at free gaps poly-X pairs score 0 matches -- candidates, never entries; diag scored
        x = strings.index("X" * 10)
        zero = [p for p, w in full[4].items() if w == 0.0 and p[0] != p[1]]
        assert full[4][(x, x)] < 0.5 and len(zero) > 0
        assert all(b not in [c for c in full[0][a] if c >= 0] for a, b in zero)
    if thr > 0:
        assert sum(degs) < sum(rows_model(n, cand["i"], cand["j"], value, 1024, 0.0, True)[3])
    for top in (1, 3, n - 1, 200, 1024):            # not clamped to n - 1: the columns behind are padding
        idx, val, diag, _, _ = rows_model(n, cand["i"], cand["j"], value, top, thr, True)
        got = da.nw_lsh_knn_dense(sig, bands, rows, top, mh_thr, value, thr)
        assert got[0].shape == (n, top) and got[2].shape == (n,)
        same_lists(got, idx, val, diag)
        assert np.array_equal(got[1] > 0, got[0] >= 0)
    for bad_top in (0, 1025):
        with pytest.raises(ValueError):
            da.nw_lsh_knn_dense(sig, bands, rows, bad_top, mh_thr, value, thr)


def test_equal_doubles_tie_whatever_their_matches_and_length(built, strings):
    """5/10 and 10/20 are one key: among equal values the column decides"""
    import dynaalign_amd as da
    sig = O.signatures(strings, 4, 48, O.seeds(12345, 48))
    pairs = {}
    for i, a in enumerate(strings):
        for j, b in enumerate(strings):
            if i < j:
                rc, mt, ln, _, _ = O.nw_pair(a, b, "BLOSUM62", 10, 4)
                pairs[(i, j)] = (mt, ln)
    value = lambda i, j: pairs[(i, j)][0] / pairs[(i, j)][1] if i != j else 1.0
    cand = model(sig, 48, 1, 0.0)
    idx, val, _ = da.nw_lsh_knn_dense(sig, 48, 1, 1024, 0.0, value)
    found = 0
    for r in range(len(strings)):
        live = idx[r] >= 0
        cols, vals = idx[r][live], val[r][live]
        assert all(vals[t] > vals[t + 1] or (vals[t] == vals[t + 1] and cols[t] < cols[t + 1]) for t in range(len(cols) - 1))
        codes = [pairs[(min(r, c), max(r, c))] for c in cols.tolist()]
        found += sum(1 for t in range(len(cols) - 1) if vals[t] == vals[t + 1] and codes[t] != codes[t + 1])
    assert found > 0 and set(zip(cand["i"], cand["j"])) >= {(min(r, c), max(r, c)) for r in range(len(strings)) for c in idx[r] if c >= 0}


def test_cross_definition_against_the_row_sort(built, strings):
    import dynaalign_amd as da
    x, y = strings[:30], strings[20:]
    sv = O.seeds(7, 40)
    sx, sy = O.signatures(x, 4, 40, sv), O.signatures(y, 4, 40, sv)
    value = nw_value_of(x, y)
    for mh_thr, thr in ((0.0, 0.0), (0.2, 0.4)):
        cand = cross_model(sx, sy, 40, 1, mh_thr)
        assert max(rows_model(len(x), cand["i"], cand["j"], value, 1024, thr, False)[3]) > 2
        for top in (1, 2, 1024):
            idx, val, _, degs, _ = rows_model(len(x), cand["i"], cand["j"], value, top, thr, False)
            got = da.nw_lsh_cross_topk_dense(sx, sy, 40, 1, top, mh_thr, value, thr)
            assert len(got) == 2 and got[0].shape == (len(x), top)
            same_lists(got, idx, val)
    # sequence1 is x: the transposed problem scores y[j] against x[i]
    back = nw_value_of(y, x)
    cand_t = cross_model(sy, sx, 40, 1, 0.0)
    idx, val, _, _, _ = rows_model(len(y), cand_t["i"], cand_t["j"], back, 5, 0.0, False)
    same_lists(da.nw_lsh_cross_topk_dense(sy, sx, 40, 1, 5, 0.0, back), idx, val)


def test_exports_and_parameter_lists():
    import dynaalign_amd as da
    from dynaalign_amd import device
    for name in ("similarityNW_lsh_knn", "similarityNW_lsh_knn_edges", "similarityNW_lsh_cross_topk", "nw_lsh_knn_dense", "nw_lsh_cross_topk_dense"):
        assert name in da.__all__ and callable(getattr(da, name)), name
    sig = inspect.signature(da.similarityNW_lsh_knn)
    assert list(sig.parameters) == ["sequences", "k", "n_hash", "bands", "rows", "top", "mh_threshold", "threshold", "matrixName", "gapOpen", "gapExt",
                                    "seed", "max_candidates"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [4, 50, 10, 5, 10, 0.0, 0.0, "BLOSUM62", 10, 4, None, 1 << 32]
    keyword_only = ("mh_threshold", "threshold", "matrixName", "gapOpen", "gapExt", "seed", "max_candidates")
    assert all(sig.parameters[p].kind is inspect.Parameter.KEYWORD_ONLY for p in keyword_only)
    edges = inspect.signature(da.similarityNW_lsh_knn_edges)
    assert list(edges.parameters) == list(sig.parameters)[:6] + ["mode"] + list(sig.parameters)[6:] and edges.parameters["mode"].default == "union"
    cross = inspect.signature(da.similarityNW_lsh_cross_topk)
    assert list(cross.parameters) == ["x", "y"] + list(sig.parameters)[1:]
    assert list(inspect.signature(da.nw_lsh_knn_dense).parameters) == ["sig", "bands", "rows", "top", "mh_threshold", "nw_value", "threshold"]
    assert list(inspect.signature(da.nw_lsh_cross_topk_dense).parameters) == ["sig_x", "sig_y", "bands", "rows", "top", "mh_threshold", "nw_value",
                                                                              "threshold"]
    assert inspect.signature(da.nw_lsh_knn_dense).parameters["threshold"].default == 0.0
    for name in ("nw_knn_select", "lsh_nw_knn", "lsh_nw_cross_topk", "nw_rank_keys"):
        assert callable(getattr(device, name)), name
    assert list(inspect.signature(device.nw_knn_select).parameters) == list(inspect.signature(device.lsh_knn_select).parameters)[:2] + \
        ["key", "top", "nnz", "out"]


@pytest.fixture(scope="module")
def lib(built):
    from dynaalign_amd import _capi
    return _capi.load()


def test_the_new_prototypes_parse_from_the_header(lib):
    import ctypes as C
    from dynaalign_amd import _capi
    declared = _capi.header_symbols()
    for name in SYMBOLS:
        assert name in declared and name in _capi.SIGNATURES and hasattr(lib, name), name
    assert sorted(_capi.SIGNATURES) == declared
    assert lib.da_abi_version() == 2                 # entry points were added, nothing changed: the version stays
    res, args = _capi.SIGNATURES["da_similarity_nw_lsh_knn"]
    p, i, q, d = C.c_void_p, C.c_int, C.c_int64, C.c_double
    assert res is C.c_int and args == [p, p, q, i, i, p, i, i, d, q, C.c_char_p, i, i, d, i, p, p, p]
    res, args = _capi.SIGNATURES["da_similarity_nw_lsh_cross_topk"]
    assert res is C.c_int and args == [p, p, q, p, p, q, i, i, p, i, i, d, q, C.c_char_p, i, i, d, i, p, p]
    res, args = _capi.SIGNATURES["da_dev_nw_knn_select"]
    assert res is C.c_int and args == _capi.SIGNATURES["da_dev_lsh_knn_select"][1] == [p, q, p, p, q, i, p, q, p, q, p]
    assert _capi.SIGNATURES["da_dev_lsh_nw_knn"][1] == [p, q, q, i, i, i, d, q, p, p, i, i, i, d, i, p, i, p, C.c_size_t, p, p, p, p]
    assert _capi.SIGNATURES["da_dev_lsh_cross_nw_topk"][1] == [p, C.c_size_t, p, q, q, p, q, q, i, i, i, d, q, p, p, p, p, i, i, i, d, i, p, i, p,
                                                               C.c_size_t, p, p, p]


def raw(lib, seqs, k=4, nh=8, bands=2, rows=4, mh_thr=0.0, maxc=1 << 32, matrix=b"BLOSUM62", thr=0.5, top=3, *, seeds=True, offsets=True, off=None,
        idx=True, val=True, diag=True, y=None, y_off=None):
    """da_similarity_nw_lsh_knn (y None) / da_similarity_nw_lsh_cross_topk through ctypes -> (status, text)"""
    res, o = O.pack(seqs)
    if off is not None:
        o = np.asarray(off, np.int64)
    sv = np.zeros(max(nh, 1), np.uint32)
    cnt = max(len(seqs), 1) * min(max(top, 1), 1024)
    out_i, out_v, out_d = np.full(cnt, -7, np.int32), np.full(cnt, -7.0), np.full(max(len(seqs), 1), -7.0)
    tail = (k, nh, sv.ctypes.data if seeds else None, bands, rows, mh_thr, maxc, matrix, 10, 4, thr, top, out_i.ctypes.data if idx else None,
            out_v.ctypes.data if val else None)
    if y is None:
        rc = lib.da_similarity_nw_lsh_knn(res.ctypes.data, o.ctypes.data if offsets else None, len(seqs), *tail, out_d.ctypes.data if diag else None)
    else:
        yres, yo = O.pack(y)
        if y_off is not None:
            yo = np.asarray(y_off, np.int64)
        rc = lib.da_similarity_nw_lsh_cross_topk(res.ctypes.data, o.ctypes.data if offsets else None, len(seqs), yres.ctypes.data, yo.ctypes.data, len(y),
                                                 *tail)
    return rc, lib.da_last_error().decode("latin-1") if rc else ""


TOP_TEXT = "top must be in 1 .. 1024 (got %d)"


def test_validation_order_and_texts(lib, kats):
    import dynaalign_amd as da
    e = kats["mh_errors"]
    two = ["ACDEFGHIK", "ACDEFGHIR"]
    nan = float("nan")
    bad_matrix = (BAD_MATRIX, "Invalid substitution matrix name: PAM250")
    # the checks of da_similarity_nw_lsh_edges_begin, in its order, with its texts; a bad top does not come before max_candidates
    assert raw(lib, [], 0, 0, 0, 0, nan, -1, b"PAM250", nan, 0, seeds=False, offsets=False, idx=False) == bad_matrix
    assert raw(lib, [], 0, 0, 0, 0, nan, -1, thr=nan, top=0, seeds=False, offsets=False, idx=False) == (EMPTY, e["empty"])
    assert raw(lib, two, 0, 0, 0, 0, nan, -1, thr=nan, top=0, seeds=False, offsets=False) == (BAD_K, e["k"])
    assert raw(lib, two, 4, 0, 0, 0, nan, -1, thr=nan, top=0, seeds=False, offsets=False) == (BAD_NHASH, e["n_hash"])
    for kw in ({"seeds": False}, {"idx": False}):
        assert raw(lib, two, 4, 8, 0, 0, nan, -1, thr=nan, top=0, off=[3, 2, 1], **kw) == (BAD_ARG, "NULL pointer"), kw
    assert raw(lib, two, 4, 8, 0, 0, nan, -1, thr=nan, top=0, offsets=False) == (BAD_ARG, "offsets is NULL")
    assert raw(lib, two, 4, 8, 0, 0, nan, -1, thr=nan, top=0, off=[0, 9, 5]) == (BAD_ARG, "offsets must be non-decreasing (sequence 1)")
    assert raw(lib, two, 4, 8, 0, 0, nan, -1, thr=nan, top=0, off=[1, 9, 18]) == (BAD_ARG, "offsets[0] must be 0")
    bad = ["ACDEFGHIK", "ACDEFGHIJ"]
    assert raw(lib, bad, 4, 8, 0, 0, nan, -1, thr=nan, top=0) == (BAD_ARG, "bands must be >= 1 (got 0)")
    assert raw(lib, bad, 4, 8, 2, 0, nan, -1, thr=nan, top=0) == (BAD_ARG, "rows must be >= 1 (got 0)")
    assert raw(lib, bad, 4, 8, 3, 4, nan, -1, thr=nan, top=0) == (BAD_ARG, "bands * rows = 12 exceeds n_hash = 8")
    assert raw(lib, bad, 4, 8, 2, 4, nan, -1, thr=nan, top=0) == (BAD_ARG, "max_candidates must be >= 0 (got -1)")
    # top: behind max_candidates, with the text of da_similarity_mh_lsh_knn, before the 16-bit limit and the residues
    for top in (0, -1, 1025):
        assert raw(lib, bad, 4, 65536, 2, 4, nan, thr=nan, top=top) == (BAD_ARG, TOP_TEXT % top)
    res, o = O.pack(two)
    sv = np.zeros(8, np.uint32)
    buf = np.zeros(8, np.float64)
    assert lib.da_similarity_mh_lsh_knn(res.ctypes.data, o.ctypes.data, 2, 4, 8, sv.ctypes.data, 2, 4, 0.0, 1025, 0, buf.ctypes.data, buf.ctypes.data) == BAD_ARG
    assert lib.da_last_error().decode() == TOP_TEXT % 1025
    assert raw(lib, bad, 4, 65536, 2, 4, nan, thr=nan) == (UNSUPPORTED, "the LSH edge list counts in 16 bits: n_hash <= 65535 (got 65536)")
    # the NW checks, then threshold, then mh_threshold
    assert raw(lib, bad, mh_thr=nan, thr=nan) == (BAD_RES2, "Invalid amino acid in sequence2: J")
    assert raw(lib, ["JCDEFGHIK", "ACDEFGHIK"], mh_thr=nan, thr=nan) == (BAD_RES1, "Invalid amino acid in sequence1: J")
    rc, text = raw(lib, ["ACDEFGHIK", "", "A" * 1025], mh_thr=nan, thr=nan)
    assert rc == UNSUPPORTED and text.startswith("sequence 2 is empty")
    rc, text = raw(lib, ["ACDEFGHIK", "A" * 1025], mh_thr=nan, thr=nan)
    assert rc == UNSUPPORTED and text == "the alignment kernels take sequences up to 1024 residues (sequence 2: 1025)"
    for v in (nan, -0.001, 1.001, float("inf")):
        assert raw(lib, two, mh_thr=nan, thr=v) == (BAD_ARG, "threshold must be in [0, 1]"), v
        assert raw(lib, two, mh_thr=v, thr=0.5) == (BAD_ARG, "mh_threshold must be in [0, 1]"), v
    # accepted (a device is needed only now): val_out and diag_out may be NULL, top is not clamped to n - 1, n = 1
    want = OK if lib.da_device_count() > 0 else NO_DEVICE
    assert raw(lib, two)[0] == want
    assert raw(lib, two, val=False, diag=False)[0] == want
    assert raw(lib, ["ACDEFGHIK", "A" * 1024], mh_thr=1.0, thr=0.0, top=1024)[0] == want
    assert raw(lib, ["ACDEFGHIK"], mh_thr=0.0, thr=1.0, maxc=0, top=1)[0] == want
    # the Python entry points pass the library's errors on
    for fn in (da.similarityNW_lsh_knn, da.similarityNW_lsh_knn_edges):
        for args, kw, code, msg in [((two,), {"matrixName": "PAM250"}, *bad_matrix), (([],), {}, EMPTY, e["empty"]),
                                    ((two, 4, 8, 3, 3), {}, BAD_ARG, "bands * rows = 9 exceeds n_hash = 8"),
                                    ((two, 4, 8, 2, 4, 0), {"max_candidates": -1}, BAD_ARG, "max_candidates must be >= 0 (got -1)"),
                                    ((two, 4, 8, 2, 4, 0), {}, BAD_ARG, TOP_TEXT % 0), ((two, 4, 8, 2, 4, 2000), {}, BAD_ARG, TOP_TEXT % 2000),
                                    ((bad, 4, 8, 2, 4), {}, BAD_RES2, "Invalid amino acid in sequence2: J"),
                                    ((two, 4, 8, 2, 4, 3), {"threshold": 1.5}, BAD_ARG, "threshold must be in [0, 1]"),
                                    ((two, 4, 8, 2, 4, 3), {"mh_threshold": -1.0}, BAD_ARG, "mh_threshold must be in [0, 1]")]:
            with pytest.raises(da.DynaAlignError) as ei:
                fn(*args, seed=1, **kw)
            assert (ei.value.code, str(ei.value)) == (code, msg), args


def test_cross_validation_order_and_texts(lib, kats):
    import dynaalign_amd as da
    e = kats["mh_errors"]
    x, y = ["ACDEFGHIK", "ACDEFGHIR"], ["ACDEFGHIK", "WCDEFGHIR", "ACDEF"]
    nan = float("nan")
    bad_matrix = (BAD_MATRIX, "Invalid substitution matrix name: PAM250")
    assert raw(lib, [], 0, 0, 0, 0, nan, -1, b"PAM250", nan, 0, y=[], seeds=False, offsets=False, idx=False) == bad_matrix
    assert raw(lib, [], 0, 0, 0, 0, nan, -1, thr=nan, top=0, y=y, seeds=False) == (EMPTY, e["empty"])
    assert raw(lib, x, 0, 0, 0, 0, nan, -1, thr=nan, top=0, y=[], seeds=False) == (EMPTY, e["empty"])
    assert raw(lib, x, 0, 0, 0, 0, nan, -1, thr=nan, top=0, y=y, seeds=False) == (BAD_K, e["k"])
    assert raw(lib, x, 4, 0, 0, 0, nan, -1, thr=nan, top=0, y=y, seeds=False) == (BAD_NHASH, e["n_hash"])
    for kw in ({"seeds": False}, {"idx": False}):
        assert raw(lib, x, 4, 8, 0, 0, nan, -1, thr=nan, top=0, y=y, off=[3, 2, 1], **kw) == (BAD_ARG, "NULL pointer"), kw
    assert raw(lib, x, 4, 8, 0, 0, nan, -1, thr=nan, top=0, y=y, off=[0, 9, 5], y_off=[1, 2, 3, 4]) == (BAD_ARG, "offsets must be non-decreasing (sequence 1)")
    assert raw(lib, x, 4, 8, 0, 0, nan, -1, thr=nan, top=0, y=y, y_off=[1, 9, 18, 23]) == (BAD_ARG, "offsets[0] must be 0")
    yb = ["ACDEFGHIK", "ACDEFGHIJ"]
    assert raw(lib, x, 4, 8, 0, 0, nan, -1, thr=nan, top=0, y=yb) == (BAD_ARG, "bands must be >= 1 (got 0)")
    assert raw(lib, x, 4, 8, 2, 0, nan, -1, thr=nan, top=0, y=yb) == (BAD_ARG, "rows must be >= 1 (got 0)")
    assert raw(lib, x, 4, 8, 3, 4, nan, -1, thr=nan, top=0, y=yb) == (BAD_ARG, "bands * rows = 12 exceeds n_hash = 8")
    assert raw(lib, x, 4, 8, 2, 4, nan, -1, thr=nan, top=0, y=yb) == (BAD_ARG, "max_candidates must be >= 0 (got -1)")
    for top in (0, 1025):
        assert raw(lib, x, 4, 65536, 2, 4, nan, thr=nan, top=top, y=yb) == (BAD_ARG, TOP_TEXT % top)
    assert raw(lib, x, 4, 65536, 2, 4, nan, thr=nan, y=yb) == (UNSUPPORTED, "the LSH edge list counts in 16 bits: n_hash <= 65535 (got 65536)")
    assert raw(lib, x, mh_thr=nan, thr=nan, y=yb) == (BAD_RES2, "Invalid amino acid in sequence2: J")
    assert raw(lib, ["JCDEFGHIK"], mh_thr=nan, thr=nan, y=yb) == (BAD_RES1, "Invalid amino acid in sequence1: J")
    rc, text = raw(lib, ["ACDEFGHIK", ""], mh_thr=nan, thr=nan, y=["A" * 1025])
    assert rc == UNSUPPORTED and text.startswith("sequence 2 of x is empty")
    rc, text = raw(lib, x, mh_thr=nan, thr=nan, y=["ACD", "", "A" * 1025])
    assert rc == UNSUPPORTED and text.startswith("sequence 2 of y is empty")
    rc, text = raw(lib, x, mh_thr=nan, thr=nan, y=["ACD", "A" * 1025])
    assert rc == UNSUPPORTED and text == "the alignment kernels take sequences up to 1024 residues (sequence 2 of y: 1025)"
    for v in (nan, -0.001, 1.001):
        assert raw(lib, x, mh_thr=nan, thr=v, y=y) == (BAD_ARG, "threshold must be in [0, 1]"), v
        assert raw(lib, x, mh_thr=v, thr=0.5, y=y) == (BAD_ARG, "mh_threshold must be in [0, 1]"), v
    want = OK if lib.da_device_count() > 0 else NO_DEVICE
    assert raw(lib, x, y=y)[0] == want
    assert raw(lib, x, y=y, val=False)[0] == want
    assert raw(lib, x, mh_thr=1.0, thr=0.0, top=1024, y=["A" * 1024])[0] == want
    with pytest.raises(da.DynaAlignError) as ei:
        da.similarityNW_lsh_cross_topk(x, y, 4, 8, 2, 4, 3, threshold=2.0, seed=1)
    assert (ei.value.code, str(ei.value)) == (BAD_ARG, "threshold must be in [0, 1]")
    with pytest.raises(da.DynaAlignError) as ei:
        da.similarityNW_lsh_cross_topk(x, y, 4, 8, 2, 4, 1025, seed=1)
    assert (ei.value.code, str(ei.value)) == (BAD_ARG, TOP_TEXT % 1025)


def test_the_device_entries_check_their_arguments_before_a_device(lib):
    p = 4096

    def select(n=4, nnz=10, top=3, ld_idx=3, ld_key=3, ptr=p, col=p, key=p, idx=p, out=p):
        return lib.da_dev_nw_knn_select(ptr, nnz, col, key, n, top, idx, ld_idx, out, ld_key, None)
    assert select(n=0) == EMPTY
    for bad_top in (0, 1025):
        assert select(top=bad_top, ld_idx=2000, ld_key=2000) == BAD_ARG and lib.da_last_error().decode() == TOP_TEXT % bad_top
    assert select(nnz=-1) == BAD_ARG and select(ld_idx=2) == BAD_ARG and select(ld_key=2) == BAD_ARG
    assert select(ptr=None) == BAD_ARG and select(idx=None) == BAD_ARG and select(out=None) == BAD_ARG and select(col=None) == BAD_ARG
    assert select(key=None) == BAD_ARG

    def keys(pairs=4, max_len=20, rank=p, totals=p, i=p):
        return lib.da_dev_nw_rank_keys(i, p, p, p, pairs, rank, max_len, 1, 1, 4, p, p, p, totals, None)
    assert keys(pairs=-1) == BAD_ARG and keys(max_len=0) == BAD_ARG and keys(max_len=1025) == BAD_ARG
    assert keys(rank=None) == BAD_ARG and keys(totals=None) == BAD_ARG and keys(i=None) == BAD_ARG
