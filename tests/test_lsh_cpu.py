"""CPU tests of MinHash LSH banding: the numpy definition (lsh_edges_dense) against an independent model, lsh_collision_probability,
exports, the C ABI's symbols, and the validation order and texts of da_similarity_mh_lsh_edges_begin -- every error arrives before a
device is needed.  On a machine without a device nothing is computed on one; on a machine with one the ACCEPTED cases of the validation
test (bands * rows == n_hash, n = 1, n_hash = 65535 as 1 x 65535, ...) run the whole pipeline on two short strings, as the accepted cases of
test_knn_abi.py do -- their results are checked in test_gpu_lsh.py, here only the status."""
import ctypes
import inspect

import numpy as np
import pytest

import oracle_lib as O

LSH_SYMBOLS = ["da_similarity_mh_lsh_edges_begin", "da_mh_lsh_last_route", "da_dev_lsh_workspace_bytes", "da_dev_lsh_band_keys",
               "da_dev_lsh_verify_pairs", "da_dev_lsh_edges"]
OK, EMPTY, BAD_K, BAD_NHASH, NO_DEVICE, UNSUPPORTED, BAD_ARG = 0, 1, 2, 3, 8, 10, 11
AA20 = "ACDEFGHIKLMNPQRSTVWY"
FIXED = ["", "A", "AC", AA20, AA20]


def model(sig, bands, rows, threshold):
    """The definition, the slow way: per band a dict from the tuple of the band's values to its members; every pair of members is a
    candidate; a candidate's count is taken column by column.  -> dict: i, j (int lists), w (Python floats), sorted by (i, j), and what
    the inputs are chosen for: incidences, pairs in >= 2 bands, candidates below the threshold, the largest bucket."""
    n, n_hash = sig.shape
    assert bands >= 1 and rows >= 1 and bands * rows <= n_hash
    seen = {}
    largest = 0
    for t in range(bands):
        buckets = {}
        for i in range(n):
            buckets.setdefault(tuple(int(v) for v in sig[i, t * rows:(t + 1) * rows]), []).append(i)
        for members in buckets.values():
            largest = max(largest, len(members))
            for a in range(len(members)):
                for b in range(a + 1, len(members)):
                    seen.setdefault((members[a], members[b]), []).append(t)
    edges = {(i, i): 1.0 for i in range(n)}
    below = 0
    for (i, j), hits in seen.items():
        c = sum(1 for h in range(n_hash) if sig[i, h] == sig[j, h]) if n_hash <= 64 else int((sig[i] == sig[j]).sum())
        assert i < j and c >= rows
        if c / n_hash >= threshold:
            edges[(i, j)] = c / n_hash
        else:
            below += 1
    order = sorted(edges)
    return {"i": [e[0] for e in order], "j": [e[1] for e in order], "w": [edges[e] for e in order],
            "incidences": sum(len(h) for h in seen.values()), "multi": sum(1 for h in seen.values() if len(h) > 1), "below": below,
            "largest": largest, "pairs": set(seen), "bands_of": seen}


def same_edges(got, want):
    i, j, w = got
    assert i.dtype == np.int32 and j.dtype == np.int32 and w.dtype == np.float64
    assert i.tolist() == want["i"] and j.tolist() == want["j"]
    assert np.array_equal(np.asarray(w).view(np.uint64), np.array(want["w"], np.float64).view(np.uint64))


def planted(seed, n, n_hash, bands, rows):
    """random uint32 signatures with planted agreements: whole-row copies, single bands copied from another row (first, last, two at once),
    a band copied but for its last column, and rows that agree in the columns behind the last band only"""
    rng = np.random.RandomState(seed)
    sig = rng.randint(0, 1 << 32, (n, n_hash), dtype=np.uint64).astype(np.uint32)
    sig[rng.rand(n, n_hash) < 0.02] = 0xFFFFFFFF
    for _ in range(n // 4):
        a, b = rng.randint(0, n, 2)
        what = rng.randint(0, 5)
        t = [0, bands - 1, rng.randint(0, bands)][rng.randint(0, 3)]
        if what == 0:
            sig[b] = sig[a]
        elif what == 1:
            sig[b, t * rows:(t + 1) * rows] = sig[a, t * rows:(t + 1) * rows]
        elif what == 2:
            sig[b, :rows] = sig[a, :rows]
            sig[b, (bands - 1) * rows:bands * rows] = sig[a, (bands - 1) * rows:bands * rows]
        elif what == 3:
            sig[b, t * rows:(t + 1) * rows - 1] = sig[a, t * rows:(t + 1) * rows - 1]
        else:
            sig[b, bands * rows:] = sig[a, bands * rows:]
    return sig


@pytest.mark.parametrize("n,n_hash,bands,rows,threshold", [(60, 24, 6, 4, 0.3), (60, 24, 5, 4, 0.0), (50, 33, 33, 1, 0.1), (50, 31, 1, 31, 0.5),
                                                           (40, 70, 3, 20, 1.0), (1, 8, 2, 4, 0.5), (2, 8, 2, 3, 0.5)])
def test_dense_definition_on_planted_signatures(n, n_hash, bands, rows, threshold):
    import dynaalign_amd as da
    sig = planted(n + n_hash, n, n_hash, bands, rows)
    want = model(sig, bands, rows, threshold)
    if n > 2:
        assert want["incidences"] > 0 and len(want["i"]) > n
    same_edges(da.lsh_edges_dense(sig, bands, rows, threshold), want)


def test_dense_definition_on_oracle_signatures(built):
    import dynaalign_amd as da
    from test_gpu_jaccard import family
    seqs = family(1, 6, 20, 120) + FIXED
    sig = O.signatures(seqs, 4, 48, O.seeds(12345, 48))
    want = model(sig, 12, 4, 0.5)
    assert want["incidences"] > 0 and want["multi"] > 0 and want["below"] > 0
    same_edges(da.lsh_edges_dense(sig, 12, 4, 0.5), want)
    for bad in [(0, 4), (12, 0), (12, 5), (49, 1)]:
        with pytest.raises(ValueError):
            da.lsh_edges_dense(sig, bad[0], bad[1], 0.5)


def test_collision_probability_hand_values():
    import dynaalign_amd as da
    p = da.lsh_collision_probability
    assert p(0.5, 1, 1) == 0.5
    assert p(0.5, 2, 1) == 0.75                 # 1 - (1 - 1/2)^2
    assert p(0.5, 1, 2) == 0.25                 # 1 - (1 - 1/4)
    assert p(0.5, 2, 2) == 0.4375               # 1 - (3/4)^2
    assert p(0.0, 10, 5) == 0.0 and p(1.0, 10, 5) == 1.0
    assert abs(p(0.8, 20, 5) - (1 - (1 - 0.32768) ** 20)) < 1e-15
    v = p(np.array([0.0, 0.5, 1.0]), 2, 2)
    assert v.tolist() == [0.0, 0.4375, 1.0]
    assert np.all(np.diff(p(np.linspace(0, 1, 50), 10, 5)) >= 0)


def test_exports_and_parameter_lists():
    import dynaalign_amd as da
    from dynaalign_amd import device, session
    for name in ("similarityMH_lsh_edges", "lsh_edges_dense", "lsh_collision_probability"):
        assert name in da.__all__ and callable(getattr(da, name)), name
    sig = inspect.signature(da.similarityMH_lsh_edges)
    assert list(sig.parameters) == ["sequences", "k", "n_hash", "bands", "rows", "threshold", "seed", "max_candidates"]
    assert [sig.parameters[p].default for p in ("k", "n_hash", "bands", "rows", "threshold", "seed", "max_candidates")] == [4, 50, 10, 5, 0.5, None, 1 << 32]
    assert sig.parameters["seed"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["max_candidates"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(da.lsh_edges_dense).parameters) == ["sig", "bands", "rows", "threshold"]
    assert list(inspect.signature(da.lsh_collision_probability).parameters) == ["s", "bands", "rows"]
    assert list(inspect.signature(device.lsh_band_keys).parameters) == ["sig", "n_hash", "bands", "rows"]
    assert list(inspect.signature(device.lsh_verify_pairs).parameters) == ["sig", "n_hash", "bands", "rows", "threshold", "i", "j", "band"]
    assert list(inspect.signature(device.lsh_edges).parameters)[:5] == ["sig", "n_hash", "bands", "rows", "threshold"]
    sig = inspect.signature(session.MinHashSession.lsh_edges)
    assert list(sig.parameters) == ["self", "bands", "rows", "threshold", "idx", "max_candidates"]
    assert sig.parameters["idx"].default is None and sig.parameters["max_candidates"].default == 1 << 32


@pytest.fixture(scope="module")
def lib(built):
    from dynaalign_amd import _capi
    return _capi.load()


def test_header_library_and_signatures_agree_on_the_lsh_symbols(lib):
    from dynaalign_amd import _capi
    declared = _capi.header_symbols()
    for name in LSH_SYMBOLS:
        assert name in declared, name
        assert name in _capi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert sorted(_capi.SIGNATURES) == declared
    assert lib.da_abi_version() == 2
    assert "#define DA_ABI_VERSION 2" in open(_capi.HEADER_PATH).read()
    assert lib.da_dev_lsh_workspace_bytes(0, 4) > 0                     # sizes need no device
    assert lib.da_dev_lsh_workspace_bytes(1000, 12) >= 1000 * 12 * (8 + 8 + 4 + 4)


def raw(lib, seqs, k, nh, bands, rows, thr, maxc=1 << 32, *, seeds=True, offsets=True, off=None, handle=True, count=True):
    """da_similarity_mh_lsh_edges_begin through ctypes -> (status, text); a handle that came back is freed"""
    res, o = O.pack(seqs)
    if off is not None:
        o = np.asarray(off, np.int64)
    sv = np.zeros(max(nh, 1), np.uint32)
    h = ctypes.c_void_p()
    cnt = np.zeros(1, np.int64)
    rc = lib.da_similarity_mh_lsh_edges_begin(res.ctypes.data, o.ctypes.data if offsets else None, len(seqs), k, nh, sv.ctypes.data if seeds else None,
                                              bands, rows, thr, maxc, ctypes.addressof(h) if handle else None, cnt.ctypes.data if count else None)
    if rc == OK:
        assert h.value and cnt[0] >= len(seqs)
        lib.da_edges_free(h)
    else:
        assert not h.value
    return rc, lib.da_last_error().decode("latin-1") if rc else ""


def test_validation_order_and_texts(lib, kats):
    import dynaalign_amd as da
    e = kats["mh_errors"]
    two = ["ACDEFGHIK", "ACDEFGHIR"]
    nan = float("nan")
    # 1-3: n, k, n_hash with the texts of similarityMH, each before everything behind it
    assert raw(lib, [], 0, 0, 0, 0, nan, -1, seeds=False, offsets=False, handle=False) == (EMPTY, e["empty"])
    assert raw(lib, two, 0, 0, 0, 0, nan, -1, seeds=False, offsets=False) == (BAD_K, e["k"])
    assert raw(lib, two, -2, 8, 2, 4, 0.5) == (BAD_K, e["k"])
    assert raw(lib, two, 4, 0, 0, 0, nan, -1, seeds=False, offsets=False) == (BAD_NHASH, e["n_hash"])
    assert raw(lib, two, 4, -5, 2, 4, 0.5) == (BAD_NHASH, e["n_hash"])
    # 4: NULL pointers, before the offsets are looked at
    for kw in ({"seeds": False}, {"handle": False}, {"count": False}):
        assert raw(lib, two, 4, 8, 0, 0, nan, -1, off=[3, 2, 1], **kw) == (BAD_ARG, "NULL pointer"), kw
    # 5: offsets, before bands / rows
    assert raw(lib, two, 4, 8, 0, 0, nan, -1, offsets=False) == (BAD_ARG, "offsets is NULL")
    assert raw(lib, two, 4, 8, 0, 0, nan, -1, off=[0, 9, 5]) == (BAD_ARG, "offsets must be non-decreasing (sequence 1)")
    assert raw(lib, two, 4, 8, 0, 0, nan, -1, off=[1, 9, 18]) == (BAD_ARG, "offsets[0] must be 0")
    # 6: bands, rows, their product, the threshold, the cap -- in this order, all before the 16-bit limit of n_hash
    for nh in (8, 70000):
        assert raw(lib, two, 4, nh, 0, 0, nan, -1) == (BAD_ARG, "bands must be >= 1 (got 0)")
        assert raw(lib, two, 4, nh, -3, 4, 0.5) == (BAD_ARG, "bands must be >= 1 (got -3)")
        assert raw(lib, two, 4, nh, 2, 0, nan, -1) == (BAD_ARG, "rows must be >= 1 (got 0)")
        assert raw(lib, two, 4, nh, nh // 4, 4, 0.5, -1)[1] == "max_candidates must be >= 0 (got -1)"
        assert raw(lib, two, 4, nh, nh // 4 + 1, 4, nan, -1) == (BAD_ARG, "bands * rows = %d exceeds n_hash = %d" % (nh + 4, nh))
        assert raw(lib, two, 4, nh, 1, nh + 1, nan, -1) == (BAD_ARG, "bands * rows = %d exceeds n_hash = %d" % (nh + 1, nh))
        for thr in (nan, -0.001, 1.001, float("inf")):
            assert raw(lib, two, 4, nh, 2, 4, thr, -1) == (BAD_ARG, "the threshold must be in [0, 1]"), thr
        assert raw(lib, two, 4, nh, 2, 4, 0.5, -1) == (BAD_ARG, "max_candidates must be >= 0 (got -1)")
    # 7: n_hash beyond the 16-bit counts, after all of the above
    assert raw(lib, two, 4, 65536, 2, 4, 0.5) == (UNSUPPORTED, "the LSH edge list counts in 16 bits: n_hash <= 65535 (got 65536)")
    # accepted: bands * rows == n_hash, the thresholds 0 and 1, a cap of 0 candidates asked of a set without any, n = 1
    want = OK if lib.da_device_count() > 0 else NO_DEVICE
    assert raw(lib, two, 4, 8, 2, 4, 0.5)[0] == want
    assert raw(lib, two, 4, 8, 8, 1, 0.0)[0] == want
    assert raw(lib, two, 4, 8, 1, 8, 1.0)[0] == want
    assert raw(lib, two, 4, 65535, 1, 65535, 0.5)[0] == want
    assert raw(lib, ["ACDEFGHIK"], 4, 8, 2, 4, 0.5, 0)[0] == want
    # the Python entry point passes the library's errors on
    for args, code, msg in [(([],), EMPTY, e["empty"]), ((two, 0), BAD_K, e["k"]), ((two, 4, 0), BAD_NHASH, e["n_hash"]),
                            ((two, 4, 8, 3, 3), BAD_ARG, "bands * rows = 9 exceeds n_hash = 8"), ((two, 4, 8, 2, 4, 1.5), BAD_ARG, "the threshold must be in [0, 1]")]:
        with pytest.raises(da.DynaAlignError) as ei:
            da.similarityMH_lsh_edges(*args, seed=1)
        assert (ei.value.code, str(ei.value)) == (code, msg), args
    with pytest.raises(da.DynaAlignError) as ei:
        da.similarityMH_lsh_edges(two, 4, 8, 2, 4, 0.5, seed=1, max_candidates=-1)
    assert ei.value.code == BAD_ARG


def test_last_route_needs_no_device_and_skips_null(lib):
    v = np.full(4, -1, np.int64)
    assert lib.da_mh_lsh_last_route(v.ctypes.data, None, None, v[3:].ctypes.data) == OK
    assert v[0] >= 0 and v[1] == -1 and v[2] == -1 and v[3] >= 0
