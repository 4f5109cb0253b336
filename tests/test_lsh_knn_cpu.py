"""CPU tests of the LSH nearest-neighbour lists: the numpy definition (lsh_knn_dense) against a pure-Python model built from
test_lsh_cpu.model's candidate pairs, exports, the C ABI's three new symbols, the validation order and texts of da_similarity_mh_lsh_knn
(every error arrives before a device is needed; on a machine with one the accepted cases run the pipeline on two short strings and only the
status is looked at -- the results are checked in test_gpu_lsh_knn.py), knn_graph on padded lists and clusterbreak's knn_lsh argument."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import oracle_lib as O
from test_lsh_cpu import FIXED, model, planted

KNN_SYMBOLS = ["da_similarity_mh_lsh_knn", "da_dev_lsh_knn", "da_dev_lsh_knn_select"]
OK, EMPTY, BAD_K, BAD_NHASH, NO_DEVICE, UNSUPPORTED, BAD_ARG = 0, 1, 2, 3, 8, 10, 11
SHAPES = [(60, 24, 6, 4), (50, 33, 33, 1), (50, 31, 1, 31), (1, 8, 2, 4)]


def knn_model(sig, bands, rows, top, threshold):
    """The definition, the slow way: the candidate pairs of test_lsh_cpu.model (its "bands_of"), a count taken column by column, per row a
    Python sort by (-count, column).  -> (idx rows, val rows, candidates per row as sorted (-count, column) lists)"""
    n, n_hash = sig.shape
    cand = [[] for _ in range(n)]
    for (i, j) in model(sig, bands, rows, threshold)["bands_of"]:
        c = sum(1 for h in range(n_hash) if sig[i, h] == sig[j, h])
        if c / n_hash >= threshold:
            cand[i].append((-c, j))
            cand[j].append((-c, i))
    idx, val = [], []
    for row in cand:
        row.sort()
        first = row[:top]
        idx.append([j for _, j in first] + [-1] * (top - len(first)))
        val.append([-c / n_hash for c, _ in first] + [0.0] * (top - len(first)))
    return idx, val, cand


def same_lists(got, want_idx, want_val):
    idx, val = got
    assert idx.dtype == np.int32 and val.dtype == np.float64 and idx.shape == val.shape == (len(want_idx), len(want_idx[0]))
    assert idx.tolist() == want_idx
    assert np.array_equal(val.view(np.uint64), np.array(want_val, np.float64).reshape(val.shape).view(np.uint64))


def test_dense_definition_against_the_python_model():
    import dynaalign_amd as da
    seen = set()
    for n, n_hash, bands, rows in SHAPES:
        sig = planted(n + n_hash, n, n_hash, bands, rows)
        cut = {4: 0.3, 1: 2 / 33, 31: 1.0}[rows]                       # removes some candidates, not all (a 1 x 31 candidate is at 1.0)
        for threshold in (0.0, cut):
            for top in (1, 3, 59):
                want_idx, want_val, cand = knn_model(sig, bands, rows, top, threshold)
                same_lists(da.lsh_knn_dense(sig, bands, rows, top, threshold), want_idx, want_val)
                # what the inputs are chosen for, from the model alone
                for row in cand:
                    seen.add(("more", top) if len(row) > top else ("none",) if not row else ("fewer", top) if len(row) < top else ("exact", top))
                    if len(row) > top and row[top - 1][0] == row[top][0]:
                        seen.add(("tie at the cut", top))               # equal counts on both sides of position top: the column decides
                    if any(a[0] == b[0] for a, b in zip(row[:top], row[1:top])):
                        seen.add(("tie in the list", top))
            if n > 1 and rows < n_hash:
                all_c = sum(len(r) for r in knn_model(sig, bands, rows, 1, 0.0)[2])
                cut_c = sum(len(r) for r in knn_model(sig, bands, rows, 1, cut)[2])
                assert 0 < cut_c < all_c, (n, n_hash, bands, rows)
    for what in [("more", 1), ("more", 3), ("fewer", 3), ("fewer", 59), ("none",), ("tie at the cut", 1), ("tie at the cut", 3), ("tie in the list", 3),
                 ("tie in the list", 59)]:
        assert what in seen, what
    # defaults and the refusals of the definition itself
    sig = planted(84, 60, 24, 6, 4)
    a, b = da.lsh_knn_dense(sig, 6, 4, 3), da.lsh_knn_dense(sig, 6, 4, 3, 0.0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for bad_top in (0, -1, 1025):
        with pytest.raises(ValueError):
            da.lsh_knn_dense(sig, 6, 4, bad_top)
    with pytest.raises(ValueError):
        da.lsh_knn_dense(sig, 7, 4, 3)
    one = da.lsh_knn_dense(planted(9, 1, 8, 2, 4), 2, 4, 1024)       # n = 1: one row of padding, top not clamped
    assert one[0].shape == (1, 1024) and (one[0] == -1).all() and (one[1] == 0.0).all()


def test_dense_definition_on_oracle_signatures(built):
    import dynaalign_amd as da
    from test_gpu_jaccard import family
    seqs = family(1, 6, 20, 120) + FIXED
    sig = O.signatures(seqs, 4, 48, O.seeds(12345, 48))
    for top in (1, 10):
        want_idx, want_val, cand = knn_model(sig, 12, 4, top, 0.0)
        assert max(len(r) for r in cand) > top and min(len(r) for r in cand) == 0
        same_lists(da.lsh_knn_dense(sig, 12, 4, top), want_idx, want_val)
        idx, val = da.lsh_knn_dense(sig, 12, 4, top)
        assert np.array_equal(val > 0, idx >= 0)                        # a value > 0 marks exactly the real entries


def test_exports_and_parameter_lists():
    import dynaalign_amd as da
    from dynaalign_amd import device, session
    for name in ("similarityMH_lsh_knn", "similarityMH_lsh_knn_edges", "lsh_knn_dense"):
        assert name in da.__all__ and callable(getattr(da, name)), name
    sig = inspect.signature(da.similarityMH_lsh_knn)
    assert list(sig.parameters) == ["sequences", "k", "n_hash", "bands", "rows", "top", "threshold", "seed", "max_candidates"]
    assert [sig.parameters[p].default for p in list(sig.parameters)[1:]] == [4, 50, 10, 5, 10, 0.0, None, 1 << 32]
    assert all(sig.parameters[p].kind is inspect.Parameter.KEYWORD_ONLY for p in ("threshold", "seed", "max_candidates"))
    sig = inspect.signature(da.similarityMH_lsh_knn_edges)
    assert list(sig.parameters) == ["sequences", "k", "n_hash", "bands", "rows", "top", "mode", "threshold", "seed", "max_candidates"]
    assert [sig.parameters[p].default for p in list(sig.parameters)[1:]] == [4, 50, 10, 5, 10, "union", 0.0, None, 1 << 32]
    assert all(sig.parameters[p].kind is inspect.Parameter.KEYWORD_ONLY for p in ("threshold", "seed", "max_candidates"))
    sig = inspect.signature(da.lsh_knn_dense)
    assert list(sig.parameters) == ["sig", "bands", "rows", "top", "threshold"] and sig.parameters["threshold"].default == 0.0
    assert list(inspect.signature(device.lsh_knn).parameters)[:5] == ["sig", "n_hash", "bands", "rows", "top"]
    assert list(inspect.signature(device.lsh_knn_select).parameters)[:4] == ["ptr", "col", "count", "top"]
    sig = inspect.signature(session.MinHashSession.lsh_knn)
    assert list(sig.parameters) == ["self", "bands", "rows", "top", "idx", "threshold", "max_candidates"]
    assert [sig.parameters[p].default for p in ("top", "idx", "threshold", "max_candidates")] == [10, None, 0.0, 1 << 32]
    sig = inspect.signature(session.MinHashSession.lsh_knn_csr)
    assert list(sig.parameters) == ["self", "bands", "rows", "idx", "top", "mode"]
    assert [sig.parameters[p].default for p in ("idx", "top", "mode")] == [None, 10, "union"]
    sig = inspect.signature(da.clusterbreak)
    assert sig.parameters["knn_lsh"].default is None and sig.parameters["knn_lsh"].kind is inspect.Parameter.KEYWORD_ONLY


def test_the_row_classes_python_names_are_the_kernels():
    """device.LSH_KNN_WAVE_MAX / LSH_KNN_LDS_WORDS, which the GPU test places its row lengths around, are the constants of lsh_kernels.hip"""
    from dynaalign_amd import device
    src = open(os.path.join(os.path.dirname(device.__file__), "csrc", "lsh_kernels.hip")).read()
    for name in ("LSH_KNN_WAVE_MAX", "LSH_KNN_LDS_WORDS"):
        found = re.findall(r"constexpr int %s = (\d+);" % name, src)
        assert found == [str(getattr(device, name))], name


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
    text = open(_capi.HEADER_PATH).read()
    assert "#define DA_ABI_VERSION 2" in text and "knn | knn_select" in text


def raw(lib, seqs, k, nh, bands, rows, thr, top, maxc=1 << 32, *, seeds=True, offsets=True, off=None, idx=True, val=True):
    """da_similarity_mh_lsh_knn through ctypes -> (status, text)"""
    res, o = O.pack(seqs)
    if off is not None:
        o = np.asarray(off, np.int64)
    sv = np.zeros(max(nh, 1), np.uint32)
    t = min(max(top, 1), 1024)
    out_i = np.full((max(len(seqs), 1), t), -7, np.int32)
    out_v = np.full((max(len(seqs), 1), t), -7.0, np.float64)
    rc = lib.da_similarity_mh_lsh_knn(res.ctypes.data, o.ctypes.data if offsets else None, len(seqs), k, nh, sv.ctypes.data if seeds else None,
                                      bands, rows, thr, top, maxc, out_i.ctypes.data if idx else None, out_v.ctypes.data if val else None)
    if rc == OK:
        assert ((out_i >= -1) & (out_i < len(seqs))).all() and ((out_v >= 0.0) & (out_v <= 1.0)).all()
    else:
        assert (out_i == -7).all() and (out_v == -7.0).all()
    return rc, lib.da_last_error().decode("latin-1") if rc else ""


def test_validation_order_and_texts(lib, kats):
    import dynaalign_amd as da
    e = kats["mh_errors"]
    two = ["ACDEFGHIK", "ACDEFGHIR"]
    nan = float("nan")
    # 1-3: n, k, n_hash with the texts of similarityMH, each before everything behind it
    assert raw(lib, [], 0, 0, 0, 0, nan, 0, -1, seeds=False, offsets=False, idx=False) == (EMPTY, e["empty"])
    assert raw(lib, two, 0, 0, 0, 0, nan, 0, -1, seeds=False, offsets=False) == (BAD_K, e["k"])
    assert raw(lib, two, -2, 8, 2, 4, 0.5, 3) == (BAD_K, e["k"])
    assert raw(lib, two, 4, 0, 0, 0, nan, 0, -1, seeds=False, offsets=False) == (BAD_NHASH, e["n_hash"])
    assert raw(lib, two, 4, -5, 2, 4, 0.5, 3) == (BAD_NHASH, e["n_hash"])
    # 4: NULL pointers, before the offsets are looked at
    for kw in ({"seeds": False}, {"idx": False}, {"val": False}):
        assert raw(lib, two, 4, 8, 0, 0, nan, 0, -1, off=[3, 2, 1], **kw) == (BAD_ARG, "NULL pointer"), kw
    # 5: offsets, before bands / rows
    assert raw(lib, two, 4, 8, 0, 0, nan, 0, -1, offsets=False) == (BAD_ARG, "offsets is NULL")
    assert raw(lib, two, 4, 8, 0, 0, nan, 0, -1, off=[0, 9, 5]) == (BAD_ARG, "offsets must be non-decreasing (sequence 1)")
    assert raw(lib, two, 4, 8, 0, 0, nan, 0, -1, off=[1, 9, 18]) == (BAD_ARG, "offsets[0] must be 0")
    # 6: bands, rows, their product, the threshold, the cap -- in this order, with the edge call's texts -- then top, all before the
    # 16-bit limit of n_hash
    for nh in (8, 70000):
        assert raw(lib, two, 4, nh, 0, 0, nan, 0, -1) == (BAD_ARG, "bands must be >= 1 (got 0)")
        assert raw(lib, two, 4, nh, -3, 4, 0.5, 0) == (BAD_ARG, "bands must be >= 1 (got -3)")
        assert raw(lib, two, 4, nh, 2, 0, nan, 0, -1) == (BAD_ARG, "rows must be >= 1 (got 0)")
        assert raw(lib, two, 4, nh, nh // 4 + 1, 4, nan, 0, -1) == (BAD_ARG, "bands * rows = %d exceeds n_hash = %d" % (nh + 4, nh))
        assert raw(lib, two, 4, nh, 1, nh + 1, nan, 0, -1) == (BAD_ARG, "bands * rows = %d exceeds n_hash = %d" % (nh + 1, nh))
        for thr in (nan, -0.001, 1.001, float("inf")):
            assert raw(lib, two, 4, nh, 2, 4, thr, 0, -1) == (BAD_ARG, "the threshold must be in [0, 1]"), thr
        assert raw(lib, two, 4, nh, 2, 4, 0.5, 0, -1) == (BAD_ARG, "max_candidates must be >= 0 (got -1)")
        for top in (0, -1, 1025):
            assert raw(lib, two, 4, nh, 2, 4, 0.5, top) == (BAD_ARG, "top must be in 1 .. 1024 (got %d)" % top)
            assert raw(lib, two, 4, nh, 2, 4, 0.5, top, -1) == (BAD_ARG, "max_candidates must be >= 0 (got -1)")
    # 7: n_hash beyond the 16-bit counts, after all of the above
    assert raw(lib, two, 4, 65536, 2, 4, 0.5, 3) == (UNSUPPORTED, "the LSH nearest-neighbour lists count in 16 bits: n_hash <= 65535 (got 65536)")
    # accepted: bands * rows == n_hash, the thresholds 0 and 1, top at both ends and beyond n - 1, a cap of 0 asked of a set without candidates, n = 1
    want = OK if lib.da_device_count() > 0 else NO_DEVICE
    assert raw(lib, two, 4, 8, 2, 4, 0.5, 1)[0] == want
    assert raw(lib, two, 4, 8, 8, 1, 0.0, 1024)[0] == want
    assert raw(lib, two, 4, 8, 1, 8, 1.0, 5)[0] == want
    assert raw(lib, two, 4, 65535, 1, 65535, 0.5, 3)[0] == want
    assert raw(lib, ["ACDEFGHIK"], 4, 8, 2, 4, 0.0, 3, 0)[0] == want
    # the Python entry points pass the library's errors on
    for args, code, msg in [(([],), EMPTY, e["empty"]), ((two, 0), BAD_K, e["k"]), ((two, 4, 0), BAD_NHASH, e["n_hash"]),
                            ((two, 4, 8, 3, 3), BAD_ARG, "bands * rows = 9 exceeds n_hash = 8"),
                            ((two, 4, 8, 2, 4, 0), BAD_ARG, "top must be in 1 .. 1024 (got 0)"),
                            ((two, 4, 8, 2, 4, 1025), BAD_ARG, "top must be in 1 .. 1024 (got 1025)")]:
        for fn in (da.similarityMH_lsh_knn, da.similarityMH_lsh_knn_edges):
            with pytest.raises(da.DynaAlignError) as ei:
                fn(*args, seed=1)
            assert (ei.value.code, str(ei.value)) == (code, msg), args
    with pytest.raises(da.DynaAlignError) as ei:
        da.similarityMH_lsh_knn(two, 4, 8, 2, 4, 3, threshold=1.5, seed=1)
    assert (ei.value.code, str(ei.value)) == (BAD_ARG, "the threshold must be in [0, 1]")
    with pytest.raises(da.DynaAlignError) as ei:
        da.similarityMH_lsh_knn(two, 4, 8, 2, 4, 3, seed=1, max_candidates=-1)
    assert ei.value.code == BAD_ARG


def test_knn_graph_drops_the_padding():
    """lists with -1 / 0.0 padding give the graph of the real entries: the padding needs no special case in knn_graph / _knn_edges_result"""
    import dynaalign_amd as da
    from dynaalign_amd.similarity import _knn_edges_result
    #          row 0: 1, 2      row 1: 0        row 2: 3 (0 lists 2, 2 does not list 0)   row 3: nothing   row 4: 2
    idx = np.array([[1, 2, -1], [0, -1, -1], [3, -1, -1], [-1, -1, -1], [2, -1, -1]], np.int32)
    val = np.array([[0.75, 0.5, 0.0], [0.75, 0.0, 0.0], [0.25, 0.0, 0.0], [0.0, 0.0, 0.0], [0.125, 0.0, 0.0]], np.float64)
    i, j, w = da.knn_graph(idx, val, None, "union")
    assert (i.tolist(), j.tolist(), w.tolist()) == ([0, 0, 2, 2], [1, 2, 3, 4], [0.75, 0.5, 0.25, 0.125])
    i, j, w = da.knn_graph(idx, val, None, "mutual")
    assert (i.tolist(), j.tolist(), w.tolist()) == ([0], [1], [0.75])
    thr, i, j, w = _knn_edges_result(idx, val, 1.0, "union")
    assert thr == 0.125 and i.min() == 0 and j.max() == 4                # no -1 reaches the edge list
    assert list(zip(i.tolist(), j.tolist(), w.tolist())) == [(0, 0, 1.0), (0, 1, 0.75), (0, 2, 0.5), (1, 1, 1.0), (2, 2, 1.0), (2, 3, 0.25), (2, 4, 0.125),
                                                              (3, 3, 1.0), (4, 4, 1.0)]
    # the same lists with the padding cut off where that is possible give the same graph
    packed = da.knn_graph(idx[:, :2], val[:, :2], 1.0, "union")
    assert all(np.array_equal(a, b) for a, b in zip(packed, (i, j, w)))
    # all padding: the diagonal alone, and a NaN in the threshold slot
    thr, i, j, w = _knn_edges_result(np.full((3, 2), -1, np.int32), np.zeros((3, 2)), 1.0, "union")
    assert thr != thr and (i.tolist(), j.tolist(), w.tolist()) == ([0, 1, 2], [0, 1, 2], [1.0, 1.0, 1.0])
    # the lists of the definition on planted signatures: every edge is a real entry of one of the two rows
    sig = planted(84, 60, 24, 6, 4)
    idx, val = da.lsh_knn_dense(sig, 6, 4, 3)
    assert (idx == -1).any()
    i, j, w = da.knn_graph(idx, val, None, "union")
    listed = {(r, int(c)) for r in range(60) for c in idx[r] if c >= 0}
    assert len(i) > 0 and all((a, b) in listed or (b, a) in listed for a, b in zip(i.tolist(), j.tolist()))
    assert {(min(a, b), max(a, b)) for a, b in listed} == set(zip(i.tolist(), j.tolist()))


def test_clusterbreak_knn_lsh_needs_a_session_and_knn():
    import dynaalign_amd as da
    pep = ["ACDEFGHIK", "ACDEFGHIR", "WWWWWYYYYY", "ACDEFGHIKL"]

    class FakeSession:
        n = len(pep)
    for kw in ({}, {"knn": 5}, {"session": FakeSession()}, {"edges_fn": lambda s: None}):
        with pytest.raises(ValueError) as e:
            da.clusterbreak(pep, knn_lsh=(12, 4), **kw)
        assert "similarityMH_lsh_knn_edges" in str(e.value) or "knn needs a session" in str(e.value), kw
    with pytest.raises(ValueError) as e:
        da.clusterbreak(pep, knn_lsh=(12, 4))
    assert "edges_fn=lambda s: similarityMH_lsh_knn_edges(" in str(e.value)
    for bad in (12, (12,), (12, 4, 1), "ab"):
        with pytest.raises(ValueError):
            da.clusterbreak(pep, session=FakeSession(), knn=2, knn_lsh=bad)
