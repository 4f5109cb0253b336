"""CPU tests of the two-set MinHash LSH form: the numpy definitions (lsh_cross_edges_dense, lsh_cross_topk_dense) against the block identity
-- the two-set result is the i < m <= j block of the one-set model on the stacked signatures --, exports, the C ABI's symbols, and the
validation order and texts of da_similarity_mh_lsh_cross_edges_begin / da_similarity_mh_lsh_cross_topk, for x and y separately: every
error arrives before a device is needed.  On a machine with a device the ACCEPTED cases of the validation test run the pipeline on short
strings; their results are checked in test_gpu_lsh_cross.py, here only the status."""
import ctypes
import inspect

import numpy as np
import pytest

import oracle_lib as O
from test_lsh_cpu import FIXED, model, planted

CROSS_SYMBOLS = ["da_dev_lsh_index_bytes", "da_dev_lsh_index_build", "da_dev_lsh_index_probe", "da_dev_lsh_cross_verify_pairs",
                 "da_dev_lsh_cross_workspace_bytes", "da_dev_lsh_cross_edges", "da_dev_lsh_cross_topk", "da_similarity_mh_lsh_cross_edges_begin",
                 "da_similarity_mh_lsh_cross_topk"]
OK, EMPTY, BAD_K, BAD_NHASH, NO_DEVICE, UNSUPPORTED, BAD_ARG = 0, 1, 2, 3, 8, 10, 11


def cross_model(sig_x, sig_y, bands, rows, threshold):
    """The two-set definition from the one-set model: model(vstack(sig_x, sig_y)) restricted to the pairs with i < m <= j, j renumbered.
    -> dict: i, j (int lists), w (Python floats) sorted by (i, j); bands_of {(i, j): agreeing bands}; incidences, multi, below as in
    test_lsh_cpu.model but of the block; largest = the longest run a query element finds; buckets = the runs of y's index"""
    m, n = len(sig_x), len(sig_y)
    n_hash = sig_x.shape[1]
    whole = model(np.vstack([sig_x, sig_y]), bands, rows, threshold)
    bands_of = {(i, j - m): t for (i, j), t in whole["bands_of"].items() if i < m <= j}
    edges = [(i, j - m, w) for i, j, w in zip(whole["i"], whole["j"], whole["w"]) if i < m <= j]
    below = sum(1 for (i, j) in bands_of if int((sig_x[i] == sig_y[j]).sum()) / n_hash < threshold)
    assert len(edges) + below == len(bands_of)
    runs = {}
    for (i, j), ts in bands_of.items():
        for t in ts:
            runs[(i, t)] = runs.get((i, t), 0) + 1
    return {"i": [e[0] for e in edges], "j": [e[1] for e in edges], "w": [e[2] for e in edges], "bands_of": bands_of, "pairs": set(bands_of),
            "incidences": sum(len(t) for t in bands_of.values()), "multi": sum(1 for t in bands_of.values() if len(t) > 1), "below": below,
            "largest": max(runs.values()) if runs else 0,
            "buckets": sum(len({tuple(r) for r in sig_y[:, t * rows:(t + 1) * rows].tolist()}) for t in range(bands))}


def topk_model(want, m, top):
    """the lists of a cross_model result: per row a Python sort by (-weight, j) -- one divide, so weight order is count order"""
    rows_ = [[] for _ in range(m)]
    for i, j, w in zip(want["i"], want["j"], want["w"]):
        rows_[i].append((-w, j))
    idx, val = [], []
    for r in rows_:
        r.sort()
        first = r[:top]
        idx.append([j for _, j in first] + [-1] * (top - len(first)))
        val.append([-w for w, _ in first] + [0.0] * (top - len(first)))
    return idx, val


def same_cross_edges(got, want):
    i, j, w = got
    assert i.dtype == np.int32 and j.dtype == np.int32 and w.dtype == np.float64
    assert i.tolist() == want["i"] and j.tolist() == want["j"]
    assert np.array_equal(np.asarray(w).view(np.uint64), np.array(want["w"], np.float64).view(np.uint64))


def same_cross_lists(got, want_idx, want_val):
    idx, val = got
    assert idx.dtype == np.int32 and val.dtype == np.float64 and idx.shape == val.shape == (len(want_idx), len(want_idx[0]))
    assert idx.tolist() == want_idx
    assert np.array_equal(val.view(np.uint64), np.array(want_val, np.float64).reshape(val.shape).view(np.uint64))


def check_definitions(da, sig_x, sig_y, bands, rows, threshold, tops=(1, 3, 40)):
    want = cross_model(sig_x, sig_y, bands, rows, threshold)
    same_cross_edges(da.lsh_cross_edges_dense(sig_x, sig_y, bands, rows, threshold), want)
    for top in tops:
        same_cross_lists(da.lsh_cross_topk_dense(sig_x, sig_y, bands, rows, top, threshold), *topk_model(want, len(sig_x), top))
    return want


@pytest.mark.parametrize("n,n_hash,bands,rows,threshold", [(60, 24, 6, 4, 0.3), (60, 24, 5, 4, 0.0), (50, 33, 33, 1, 0.1), (50, 31, 1, 31, 0.5),
                                                           (40, 70, 3, 20, 1.0), (2, 8, 2, 3, 0.5)])
def test_dense_definitions_are_the_block_of_the_one_set_model(n, n_hash, bands, rows, threshold):
    import dynaalign_amd as da
    sig = planted(n + n_hash, n, n_hash, bands, rows)
    found = 0
    for m in sorted({1, max(n // 3, 1), n // 2, n - 1}):            # split points: one query, one resident row, and in between
        want = check_definitions(da, sig[:m], sig[m:], bands, rows, threshold)
        found += want["incidences"]
        # the other way round is the transposed set
        back = da.lsh_cross_edges_dense(sig[m:], sig[:m], bands, rows, threshold)
        assert sorted(zip(back[1].tolist(), back[0].tolist())) == list(zip(want["i"], want["j"]))
    if n > 2:
        assert found > 0


def test_dense_definitions_on_oracle_signatures(built):
    import dynaalign_amd as da
    from test_gpu_jaccard import family
    fam = family(1, 6, 20, 120)
    x, y = fam[:50] + FIXED, fam[50:] + FIXED                       # the fixed strings on both sides: byte-identical pairs across the sets
    seeds = O.seeds(12345, 48)
    sig_x, sig_y = O.signatures(x, 4, 48, seeds), O.signatures(y, 4, 48, seeds)
    want = check_definitions(da, sig_x, sig_y, 12, 4, 0.5)
    assert want["incidences"] > 0 and want["multi"] > 0 and want["below"] > 0
    assert (len(x) - 1, len(y) - 1) in want["pairs"] and 1.0 in want["w"]
    for bad in [(0, 4), (12, 0), (12, 5), (49, 1)]:
        with pytest.raises(ValueError):
            da.lsh_cross_edges_dense(sig_x, sig_y, bad[0], bad[1], 0.5)
    with pytest.raises(ValueError):
        da.lsh_cross_edges_dense(sig_x, sig_y[:, :40], 10, 4, 0.5)
    for top in (0, 1025):
        with pytest.raises(ValueError):
            da.lsh_cross_topk_dense(sig_x, sig_y, 12, 4, top)
    # nothing in common: empty list, all padding
    i, j, w = da.lsh_cross_edges_dense(sig_x[:3], sig_y[:3] ^ np.uint32(1), 12, 4, 0.0)
    assert len(i) == len(j) == len(w) == 0
    idx, val = da.lsh_cross_topk_dense(sig_x[:3], sig_y[:3] ^ np.uint32(1), 12, 4, 5)
    assert (idx == -1).all() and (val == 0.0).all() and idx.shape == (3, 5)


def test_exports_and_parameter_lists():
    import dynaalign_amd as da
    from dynaalign_amd import device, session
    for name in ("similarityMH_lsh_cross_edges", "similarityMH_lsh_cross_topk", "lsh_cross_edges_dense", "lsh_cross_topk_dense"):
        assert name in da.__all__ and callable(getattr(da, name)), name
    sig = inspect.signature(da.similarityMH_lsh_cross_edges)
    assert list(sig.parameters) == ["x", "y", "k", "n_hash", "bands", "rows", "threshold", "seed", "max_candidates"]
    assert [sig.parameters[p].default for p in ("k", "n_hash", "bands", "rows", "threshold", "seed", "max_candidates")] == [4, 50, 10, 5, 0.5, None, 1 << 32]
    assert sig.parameters["seed"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["max_candidates"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(da.similarityMH_lsh_cross_topk)
    assert list(sig.parameters) == ["x", "y", "k", "n_hash", "bands", "rows", "top", "threshold", "seed", "max_candidates"]
    assert [sig.parameters[p].default for p in ("k", "n_hash", "bands", "rows", "top", "threshold", "seed", "max_candidates")] == [4, 50, 10, 5, 10, 0.0, None, 1 << 32]
    assert all(sig.parameters[p].kind is inspect.Parameter.KEYWORD_ONLY for p in ("threshold", "seed", "max_candidates"))
    assert list(inspect.signature(da.lsh_cross_edges_dense).parameters) == ["sig_x", "sig_y", "bands", "rows", "threshold"]
    sig = inspect.signature(da.lsh_cross_topk_dense)
    assert list(sig.parameters) == ["sig_x", "sig_y", "bands", "rows", "top", "threshold"] and sig.parameters["threshold"].default == 0.0
    for name in ("lsh_index_bytes", "lsh_index_build", "lsh_index_probe", "lsh_cross_verify_pairs", "lsh_cross_edges", "lsh_cross_topk"):
        assert callable(getattr(device, name)), name
    assert list(inspect.signature(device.lsh_index_bytes).parameters) == ["n", "bands"]
    assert list(inspect.signature(device.lsh_index_build).parameters)[:4] == ["sig_y", "n_hash", "bands", "rows"]
    assert list(inspect.signature(device.lsh_cross_edges).parameters)[:7] == ["index", "sig_x", "sig_y", "n_hash", "bands", "rows", "threshold"]
    assert list(inspect.signature(device.lsh_cross_topk).parameters)[:7] == ["index", "sig_x", "sig_y", "n_hash", "bands", "rows", "top"]
    cls = session.MinHashSession
    sig = inspect.signature(cls.lsh_index)
    assert list(sig.parameters) == ["self", "bands", "rows", "idx"] and sig.parameters["idx"].default is None
    sig = inspect.signature(cls.lsh_cross_edges)
    assert list(sig.parameters) == ["self", "sequences", "bands", "rows", "threshold", "idx", "max_candidates"]
    assert sig.parameters["idx"].default is None and sig.parameters["max_candidates"].default == 1 << 32
    sig = inspect.signature(cls.lsh_cross_topk)
    assert list(sig.parameters) == ["self", "sequences", "bands", "rows", "top", "idx", "threshold", "max_candidates"]
    assert [sig.parameters[p].default for p in ("top", "idx", "threshold", "max_candidates")] == [10, None, 0.0, 1 << 32]


@pytest.fixture(scope="module")
def lib(built):
    from dynaalign_amd import _capi
    return _capi.load()


def test_header_library_and_signatures_agree_on_the_cross_symbols(lib):
    from dynaalign_amd import _capi
    declared = _capi.header_symbols()
    for name in CROSS_SYMBOLS:
        assert name in declared, name
        assert name in _capi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert sorted(_capi.SIGNATURES) == declared
    assert lib.da_abi_version() == 2
    assert "#define DA_ABI_VERSION 2" in open(_capi.HEADER_PATH).read()
    assert lib.da_dev_lsh_index_bytes(0, 4) > 0                         # sizes need no device
    assert lib.da_dev_lsh_index_bytes(1000, 12) >= 1000 * 12 * (8 + 4) + 13 * 4
    assert lib.da_dev_lsh_cross_workspace_bytes(0, 4) > 0
    assert lib.da_dev_lsh_cross_workspace_bytes(1000, 12) >= 1000 * 12 * (4 + 8 + 8)


def raw(lib, what, x, y, k, nh, bands, rows, thr, maxc=1 << 32, top=5, *, seeds=True, xoff=True, yoff=True, xo=None, yo=None, xres=True, yres=True,
        out1=True, out2=True):
    """da_similarity_mh_lsh_cross_edges_begin (what = "edges") or da_similarity_mh_lsh_cross_topk ("topk") through ctypes -> (status, text);
    a handle that came back is freed"""
    (xr, xoffs), (yr, yoffs) = O.pack(x), O.pack(y)
    if xo is not None:
        xoffs = np.asarray(xo, np.int64)
    if yo is not None:
        yoffs = np.asarray(yo, np.int64)
    sv = np.zeros(max(nh, 1), np.uint32)
    front = (xr.ctypes.data if xres else None, xoffs.ctypes.data if xoff else None, len(x), yr.ctypes.data if yres else None,
             yoffs.ctypes.data if yoff else None, len(y), k, nh, sv.ctypes.data if seeds else None, bands, rows, thr)
    if what == "edges":
        h = ctypes.c_void_p()
        cnt = np.full(1, -1, np.int64)
        rc = lib.da_similarity_mh_lsh_cross_edges_begin(*front, maxc, ctypes.addressof(h) if out1 else None, cnt.ctypes.data if out2 else None)
        if rc == OK:
            assert h.value and cnt[0] >= 0
            lib.da_edges_free(h)
        else:
            assert not h.value
    else:
        t = min(max(top, 1), 1024)
        idx, val = np.zeros((max(len(x), 1), t), np.int32), np.zeros((max(len(x), 1), t), np.float64)
        rc = lib.da_similarity_mh_lsh_cross_topk(*front, top, maxc, idx.ctypes.data if out1 else None, val.ctypes.data if out2 else None)
    return rc, lib.da_last_error().decode("latin-1") if rc else ""


@pytest.mark.parametrize("what", ["edges", "topk"])
def test_validation_order_and_texts(lib, kats, what):
    e = kats["mh_errors"]
    two, one = ["ACDEFGHIK", "ACDEFGHIR"], ["ACDEFGHIK"]
    nan = float("nan")
    call = lambda *a, **kw: raw(lib, what, *a, **kw)
    # 1: x empty, then y empty, each before everything behind it (k, n_hash, pointers)
    assert call([], [], 0, 0, 0, 0, nan, -1, seeds=False, xoff=False, yoff=False, out1=False) == (EMPTY, e["empty"])
    assert call([], two, 0, 0, 0, 0, nan, -1, seeds=False) == (EMPTY, e["empty"])
    assert call(two, [], 0, 0, 0, 0, nan, -1, seeds=False) == (EMPTY, e["empty"])
    # 2-3: k, n_hash with the texts of similarityMH
    assert call(two, one, 0, 0, 0, 0, nan, -1, seeds=False, xoff=False) == (BAD_K, e["k"])
    assert call(two, one, -2, 8, 2, 4, 0.5) == (BAD_K, e["k"])
    assert call(two, one, 4, 0, 0, 0, nan, -1, seeds=False, yoff=False) == (BAD_NHASH, e["n_hash"])
    assert call(two, one, 4, -5, 2, 4, 0.5) == (BAD_NHASH, e["n_hash"])
    # 4: NULL pointers, before the offsets are looked at
    for kw in ({"seeds": False}, {"out1": False}, {"out2": False}, {"xres": False}, {"yres": False}):
        assert call(two, one, 4, 8, 0, 0, nan, -1, xo=[3, 2, 1], **kw) == (BAD_ARG, "NULL pointer"), kw
    # 5: the offsets of x, then those of y, before bands / rows
    assert call(two, one, 4, 8, 0, 0, nan, -1, xoff=False, yoff=False) == (BAD_ARG, "offsets is NULL")
    assert call(two, two, 4, 8, 0, 0, nan, -1, xo=[0, 9, 5], yo=[1, 9, 18]) == (BAD_ARG, "offsets must be non-decreasing (sequence 1)")
    assert call(two, two, 4, 8, 0, 0, nan, -1, xo=[1, 9, 18], yo=[0, 9, 5]) == (BAD_ARG, "offsets[0] must be 0")
    assert call(two, two, 4, 8, 0, 0, nan, -1, yoff=False) == (BAD_ARG, "offsets is NULL")
    assert call(two, two, 4, 8, 0, 0, nan, -1, yo=[0, 9, 5]) == (BAD_ARG, "offsets must be non-decreasing (sequence 1)")
    assert call(two, two, 4, 8, 0, 0, nan, -1, yo=[1, 9, 18]) == (BAD_ARG, "offsets[0] must be 0")
    # 6: bands, rows, their product, the threshold, the cap, top -- the order and texts of the one-set calls, before the 16-bit limit
    for nh in (8, 70000):
        assert call(two, one, 4, nh, 0, 0, nan, -1, 0) == (BAD_ARG, "bands must be >= 1 (got 0)")
        assert call(two, one, 4, nh, -3, 4, 0.5) == (BAD_ARG, "bands must be >= 1 (got -3)")
        assert call(two, one, 4, nh, 2, 0, nan, -1, 0) == (BAD_ARG, "rows must be >= 1 (got 0)")
        assert call(two, one, 4, nh, nh // 4 + 1, 4, nan, -1, 0) == (BAD_ARG, "bands * rows = %d exceeds n_hash = %d" % (nh + 4, nh))
        assert call(two, one, 4, nh, 1, nh + 1, nan, -1, 0) == (BAD_ARG, "bands * rows = %d exceeds n_hash = %d" % (nh + 1, nh))
        for thr in (nan, -0.001, 1.001, float("inf")):
            assert call(two, one, 4, nh, 2, 4, thr, -1, 0) == (BAD_ARG, "the threshold must be in [0, 1]"), thr
        assert call(two, one, 4, nh, 2, 4, 0.5, -1, 0) == (BAD_ARG, "max_candidates must be >= 0 (got -1)")
        if what == "topk":
            for top in (0, -1, 1025):
                assert call(two, one, 4, nh, 2, 4, 0.5, 0, top) == (BAD_ARG, "top must be in 1 .. 1024 (got %d)" % top)
    # 7: n_hash beyond the 16-bit counts, after all of the above
    noun = "edge list counts" if what == "edges" else "nearest-neighbour lists count"
    assert call(two, one, 4, 65536, 2, 4, 0.5) == (UNSUPPORTED, "the LSH %s in 16 bits: n_hash <= 65535 (got 65536)" % noun)
    # accepted: bands * rows == n_hash, the thresholds 0 and 1, a cap of 0 candidates asked of sets without any, m = n = 1, top beyond n
    want = OK if lib.da_device_count() > 0 else NO_DEVICE
    assert call(two, one, 4, 8, 2, 4, 0.5)[0] == want
    assert call(two, two, 4, 8, 8, 1, 0.0)[0] == want
    assert call(one, two, 4, 8, 1, 8, 1.0, top=1024)[0] == want
    assert call(one, ["WWWWWYYYYY"], 4, 8, 2, 4, 0.5, 0)[0] == want


def test_python_entry_points_pass_the_errors_on(lib, kats):
    import dynaalign_amd as da
    e = kats["mh_errors"]
    two = ["ACDEFGHIK", "ACDEFGHIR"]
    for fn in (da.similarityMH_lsh_cross_edges, da.similarityMH_lsh_cross_topk):
        for args, code, msg in [(([], two), EMPTY, e["empty"]), ((two, []), EMPTY, e["empty"]), ((two, two, 0), BAD_K, e["k"]),
                                ((two, two, 4, 0), BAD_NHASH, e["n_hash"]), ((two, two, 4, 8, 3, 3), BAD_ARG, "bands * rows = 9 exceeds n_hash = 8")]:
            with pytest.raises(da.DynaAlignError) as ei:
                fn(*args, seed=1)
            assert (ei.value.code, str(ei.value)) == (code, msg), args
        with pytest.raises(da.DynaAlignError) as ei:
            fn(two, two, 4, 8, 2, 4, seed=1, max_candidates=-1)
        assert ei.value.code == BAD_ARG
    with pytest.raises(da.DynaAlignError) as ei:
        da.similarityMH_lsh_cross_edges(two, two, 4, 8, 2, 4, 1.5, seed=1)
    assert str(ei.value) == "the threshold must be in [0, 1]"
    with pytest.raises(da.DynaAlignError) as ei:
        da.similarityMH_lsh_cross_topk(two, two, 4, 8, 2, 4, 1025, seed=1)
    assert str(ei.value) == "top must be in 1 .. 1024 (got 1025)"
