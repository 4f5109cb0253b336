"""CPU tests of the two-set top-k boundary (similarityMH_cross_topk / similarityNW_cross_topk, da_dev_topk_rows, the one-call device
route): symbols, validation order and texts (those of the *_cross calls, then the checks on `top`), the NW value-rank table, and a numpy
model of the algorithm the selection kernel implements (radix select on two 8-bit digits, ordered compaction, sort of the candidates)
against numpy's stable argsort.  No compute calls here."""
import numpy as np
import pytest

import oracle_lib as O

TOPK_SYMBOLS = ["da_similarity_mh_cross_topk", "da_similarity_nw_cross_topk", "da_dev_topk_rows", "da_dev_similarity_mh_cross_topk",
                "da_nw_code_ranks"]
OK, EMPTY, BAD_K, BAD_NHASH, BAD_MATRIX, NO_DEVICE, UNSUPPORTED, BAD_ARG = 0, 1, 2, 3, 4, 8, 10, 11


@pytest.fixture(scope="module")
def lib(built):
    from dynaalign_amd import _capi
    return _capi.load()


def test_header_library_and_signatures_agree_on_the_topk_symbols(lib):
    from dynaalign_amd import _capi
    declared = _capi.header_symbols()
    for name in TOPK_SYMBOLS:
        assert name in declared, name
        assert name in _capi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert sorted(_capi.SIGNATURES) == declared
    assert lib.da_abi_version() == 2


def test_python_mirror_exports():
    import inspect
    import dynaalign_amd as da
    from dynaalign_amd import device, session
    sig = inspect.signature(da.similarityMH_cross_topk)
    assert list(sig.parameters) == ["x", "y", "k", "n_hash", "top", "seed"]
    assert [sig.parameters[p].default for p in ("k", "n_hash", "top", "seed")] == [4, 50, 10, None]
    assert sig.parameters["seed"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(da.similarityNW_cross_topk)
    assert list(sig.parameters) == ["x", "y", "matrixName", "gapOpen", "gapExt", "top"]
    assert [sig.parameters[p].default for p in ("matrixName", "gapOpen", "gapExt", "top")] == ["BLOSUM62", 10, 4, 10]
    assert callable(device.topk_rows) and callable(device.similarity_mh_cross_topk)
    sig = inspect.signature(session.MinHashSession.cross_topk)
    assert list(sig.parameters)[:4] == ["self", "sequences", "top", "idx"] and sig.parameters["top"].default == 10
    assert callable(session.MinHashSession._joint_operand)          # cross and cross_topk share the joint-operand construction


def raw_mh(lib, x, y, k, nh, top, with_val=True):
    xr, xo = O.pack(x)
    yr, yo = O.pack(y)
    seeds = np.zeros(max(nh, 1), np.uint32)
    cnt = max(len(x), 1) * max(top, 1)
    idx, val = np.full(cnt, -7, np.int32), np.full(cnt, -7.0)
    rc = lib.da_similarity_mh_cross_topk(xr.ctypes.data, xo.ctypes.data, len(x), yr.ctypes.data, yo.ctypes.data, len(y), k, nh,
                                         seeds.ctypes.data, top, idx.ctypes.data, val.ctypes.data if with_val else None)
    return rc, lib.da_last_error().decode("latin-1") if rc else ""


def raw_nw(lib, x, y, top, matrix=b"BLOSUM62"):
    xr, xo = O.pack(x)
    yr, yo = O.pack(y)
    cnt = max(len(x), 1) * max(top, 1)
    idx, val = np.full(cnt, -7, np.int32), np.full(cnt, -7.0)
    rc = lib.da_similarity_nw_cross_topk(xr.ctypes.data, xo.ctypes.data, len(x), yr.ctypes.data, yo.ctypes.data, len(y), matrix, 10, 4, top,
                                         idx.ctypes.data, val.ctypes.data)
    return rc, lib.da_last_error().decode("latin-1") if rc else ""


def test_mh_validation_is_that_of_the_cross_call_then_top(lib, kats):
    import dynaalign_amd as da
    e = kats["mh_errors"]
    # x empty, then y empty, then k, then n_hash -- whatever top is; the texts are those of similarityMH_cross
    for x, y, k, nh, code, msg in [([], [], 0, 0, EMPTY, e["empty"]), ([], ["ACDE"], 0, 0, EMPTY, e["empty"]), (["ACDE"], [], 0, 0, EMPTY, e["empty"]),
                                   (["ACDE"], ["ACDE"], 0, 0, BAD_K, e["k"]), (["ACDE"], ["ACDE"], -1, 5, BAD_K, e["k"]),
                                   (["ACDE"], ["ACDE"], 4, 0, BAD_NHASH, e["n_hash"]), (["ACDE"], ["ACDE"], 4, -3, BAD_NHASH, e["n_hash"])]:
        for top in (0, 1, 5000):
            with pytest.raises(da.DynaAlignError) as ei:
                da.similarityMH_cross_topk(x, y, k, nh, top)
            assert (ei.value.code, str(ei.value)) == (code, msg), (x, y, k, nh, top)
            with pytest.raises(da.DynaAlignError) as ej:
                da.similarityMH_cross(x, y, k, nh)
            assert (ej.value.code, str(ej.value)) == (code, msg)
            assert raw_mh(lib, x, y, k, nh, top) == (code, msg)
    # the 16-bit limit comes before top, as in the cross call it comes before the device
    assert raw_mh(lib, ["ACDE"], ["ACDE"], 4, 70000, 0)[0] == UNSUPPORTED
    # the device form validates alike, before it looks at a pointer
    for m, n, k, nh, code in [(0, 0, 0, 0, EMPTY), (0, 3, 4, 8, EMPTY), (3, 0, 4, 8, EMPTY), (3, 3, 0, 0, BAD_K), (3, 3, 4, 0, BAD_NHASH)]:
        assert lib.da_dev_similarity_mh_cross_topk(None, None, m, None, None, n, k, nh, None, 1, None, None, 1, None) == code
    assert lib.da_dev_similarity_mh_cross_topk(None, None, 3, None, None, 3, 4, 8, None, 1, None, None, 1, None) == BAD_ARG


def test_top_out_of_range(lib):
    y = ["ACDEFGHIK"] * 3
    assert raw_mh(lib, ["ACDE"], y, 4, 8, 0)[0] == BAD_ARG
    assert raw_mh(lib, ["ACDE"], y, 4, 8, -1)[0] == BAD_ARG
    assert raw_mh(lib, ["ACDE"], y, 4, 8, 4)[0] == BAD_ARG                      # n + 1: the C ABI does not clamp
    assert raw_nw(lib, ["ACDE"], y, 0)[0] == BAD_ARG
    assert raw_nw(lib, ["ACDE"], y, 4)[0] == BAD_ARG
    big = ["ACDEFGHIK"] * 1025
    rc, msg = raw_mh(lib, ["ACDE"], big, 4, 8, 1025)
    assert rc == UNSUPPORTED and "1024" in msg
    rc, msg = raw_nw(lib, ["ACDE"], big, 1025)
    assert rc == UNSUPPORTED and "1024" in msg
    assert raw_mh(lib, ["ACDE"], big, 4, 8, 1026)[0] == BAD_ARG                 # beyond n first
    # the selection call itself (no pointer is dereferenced by these)
    p = 4096

    def tk(rows=4, n=100, ld=104, top=10, ld_out=10, keys=p, idx=p, key=p, bits=0):
        return lib.da_dev_topk_rows(keys, rows, n, ld, None, bits, top, idx, key, ld_out, None)
    assert tk(top=0) == BAD_ARG and tk(top=101) == BAD_ARG and tk(ld=99) == BAD_ARG and tk(ld_out=9) == BAD_ARG
    assert tk(keys=None) == BAD_ARG and tk(idx=None) == BAD_ARG and tk(key=None) == BAD_ARG and tk(bits=17) == BAD_ARG
    assert tk(n=2000, ld=2000, top=1025, ld_out=1025) == UNSUPPORTED
    assert tk(rows=0) == OK
    # device one-call: top after the MinHash validation
    assert lib.da_dev_similarity_mh_cross_topk(p, p, 3, p, p, 3, 4, 8, p, 4, p, p, 4, None) == BAD_ARG
    assert lib.da_dev_similarity_mh_cross_topk(p, p, 3, p, p, 2000, 4, 8, p, 1025, p, p, 1025, None) == UNSUPPORTED
    assert lib.da_dev_similarity_mh_cross_topk(p, p, 3, p, p, 3, 4, 8, p, 2, p, p, 1, None) == BAD_ARG      # ld_out < top


def test_python_mirror_clamps_top(lib):
    import dynaalign_amd as da
    # top = 5 against 2 sequences passes validation (clamped to 2): the call gets as far as the device
    for call in (lambda: da.similarityMH_cross_topk(["ACDEFG"], ["ACDEFG", "ACDEFH"], 4, 8, 5, seed=1),
                 lambda: da.similarityNW_cross_topk(["ACDEFG"], ["ACDEFG", "ACDEFH"], top=5)):
        if lib.da_device_count() > 0:
            idx, val = call()
            assert idx.shape == (1, 2) and val.shape == (1, 2) and idx.dtype == np.int32 and val.dtype == np.float64
        else:
            with pytest.raises(da.DynaAlignError) as ei:
                call()
            assert ei.value.code == NO_DEVICE


def test_nw_validation(lib, kats):
    import dynaalign_amd as da
    for x, y in [(["AA"], ["AA"]), ([], ["AA"]), (["AA"], []), (["AJ"], ["JJ"])]:
        with pytest.raises(da.DynaAlignError) as ei:
            da.similarityNW_cross_topk(x, y, "PAM250")
        assert (ei.value.code, str(ei.value)) == (BAD_MATRIX, kats["nw_bad_matrix"]["error"])
    # m == 0: DA_OK, nothing written; n == 0 with m > 0: no top can satisfy 1 <= top <= 0
    idx, val = da.similarityNW_cross_topk([], ["AA"], top=1)
    assert idx.shape == (0, 1) and val.shape == (0, 1)
    assert raw_nw(lib, [], ["J"], 1)[0] == OK and raw_nw(lib, [], [], 1)[0] == OK
    assert raw_nw(lib, ["AA"], [], 1)[0] == BAD_ARG
    # residue errors are those of da_similarity_nw_cross, unchanged, and come before top and before the empty-sequence refusal
    for x, y, code, msg in [(["AJ"], ["AA"], O.ERR_BAD_RES1, "Invalid amino acid in sequence1: J"),
                            (["AA"], ["AJ"], O.ERR_BAD_RES2, "Invalid amino acid in sequence2: J"),
                            (["", "JA"], ["AA"], O.ERR_BAD_RES1, "Invalid amino acid in sequence1: J"),
                            (["A"], ["J", "AA"], O.ERR_BAD_RES2, "Invalid amino acid in sequence2: J"),
                            (["AA", "AJ"], ["AA", "AU"], O.ERR_BAD_RES2, "Invalid amino acid in sequence2: U")]:
        for top in (0, 1):
            assert raw_nw(lib, x, y, top) == (code, msg), (x, y, top)
    # an empty sequence on either side is refused with a message; so is a sequence beyond the 8-bit alignment length
    for x, y, who in [(["AA", ""], ["AA"], "sequence 2 of x"), (["AA"], ["AC", "AA", ""], "sequence 3 of y")]:
        rc, msg = raw_nw(lib, x, y, 1)
        assert rc == UNSUPPORTED and who in msg and "empty" in msg and "NaN" in msg, msg
    rc, msg = raw_nw(lib, ["A" * 128], ["AA"], 1)
    assert rc == UNSUPPORTED and "127" in msg
    # top is checked before those limits
    assert raw_nw(lib, ["AA", ""], ["AA"], 0)[0] == BAD_ARG


def test_valid_input_fails_loudly_without_a_device(lib):
    if lib.da_device_count() > 0:
        assert raw_mh(lib, ["ACDEFG", "ACDEFH"], ["ACDEFG", "ACDEFH"], 4, 8, 2)[0] == OK
        assert raw_mh(lib, ["ACDEFG", "ACDEFH"], ["ACDEFG", "ACDEFH"], 4, 8, 2, with_val=False)[0] == OK
        assert raw_nw(lib, ["ACD", "AC"], ["AC", "A"], 2)[0] == OK
        return
    rc, msg = raw_mh(lib, ["ACDEFG", "ACDEFH"], ["ACDEFG", "ACDEFH"], 4, 8, 2)
    assert rc == NO_DEVICE and "no CPU fallback" in msg
    assert raw_mh(lib, ["ACDEFG", "ACDEFH"], ["ACDEFG", "ACDEFH"], 4, 8, 2, with_val=False)[0] == NO_DEVICE
    assert raw_nw(lib, ["ACD", "AC"], ["AC", "A"], 2)[0] == NO_DEVICE


# ---- the NW value-rank table ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_len", [1, 2, 7, 30, 127])
def test_nw_rank_table(lib, max_len):
    import dynaalign_amd as da
    ranks, distinct = da.nw_code_ranks(max_len)
    assert ranks.dtype == np.uint16 and ranks.shape == (65536,)
    code = np.arange(65536)
    mt, ln = code >> 8, code & 255
    valid = (ln >= 1) & (ln <= 2 * max_len) & (mt <= np.minimum(ln, max_len))
    value = mt[valid].astype(np.float64) / ln[valid].astype(np.float64)          # the divide of the library, IEEE on both sides
    r = ranks[valid].astype(np.int64)
    # dense ranks of the double: equal doubles <=> equal ranks, larger double <=> larger rank
    uniq, dense = np.unique(value, return_inverse=True)
    assert np.array_equal(r, dense)
    assert distinct == len(uniq) == int(r.max()) + 1 and distinct <= 65536
    order = np.argsort(value, kind="stable")
    dv, dr = np.diff(value[order]), np.diff(r[order])
    assert np.array_equal(dv > 0, dr > 0) and np.array_equal(dv == 0, dr == 0)
    assert not ranks[~valid].any()                                                # codes that cannot occur: rank 0
    if max_len >= 3:
        assert ranks[(2 << 8) | 4] == ranks[(3 << 8) | 6] == ranks[(1 << 8) | 2]   # 2/4, 3/6, 1/2: different codes, one value
        assert ranks[(2 << 8) | 4] > ranks[(1 << 8) | 3] > ranks[(0 << 8) | 5] == 0
        assert ranks[(3 << 8) | 3] == distinct - 1                                # 1.0 is the top rank


def test_nw_rank_table_refuses_bad_arguments(lib):
    out = np.zeros(65536, np.uint16)
    assert lib.da_nw_code_ranks(0, out.ctypes.data, None) == BAD_ARG
    assert lib.da_nw_code_ranks(128, out.ctypes.data, None) == BAD_ARG
    assert lib.da_nw_code_ranks(5, None, None) == BAD_ARG
    assert lib.da_nw_code_ranks(5, out.ctypes.data, None) == OK


# ---- a numpy model of k_topk_rows ----------------------------------------------------------------------------------------------------------

def model_topk(rank_row, top, rank_bits, chunk=2048):
    """What the kernel does with one row of ranks: (1) histogram of the high digit (the top 8 of rank_bits), read from the top, then of
    the low digit inside that bin -> T, the rank of the top-th element, and `above`, the elements above it; (2) chunk by chunk, in column
    order: every element above T, and the first top - above elements equal to T; (3) the candidates sorted as words rank : ~column."""
    r = np.asarray(rank_row, np.int64)
    shift = max(rank_bits - 8, 0)

    def pick(hist, want):                       # the bin holding the want-th largest element, and the count in the bins above it
        acc = 0
        for b in range(255, -1, -1):
            if acc < want <= acc + hist[b]:
                return b, acc
            acc += hist[b]
        raise AssertionError("fewer than `want` elements")
    B, above = pick(np.bincount(np.minimum(r >> shift, 255), minlength=256), top)
    T = B
    if shift:
        b, above_lo = pick(np.bincount(r[(r >> shift) == B] & ((1 << shift) - 1), minlength=256), top - above)
        T, above = (B << shift) | b, above + above_lo
    need_eq = top - above
    assert need_eq >= 1
    cand = np.zeros(top, np.uint64)
    gt_run = eq_run = 0
    for c0 in range(0, len(r), chunk):
        seg = r[c0:c0 + chunk]
        gt, eq = seg > T, seg == T
        gt_at = gt_run + np.cumsum(gt) - gt       # exclusive prefix: the slot of every element above T
        eq_at = eq_run + np.cumsum(eq) - eq
        j = np.arange(c0, c0 + len(seg), dtype=np.uint64)
        word = (seg.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - j)
        cand[gt_at[gt]] = word[gt]
        take = eq & (eq_at < need_eq)
        cand[above + eq_at[take]] = word[take]
        gt_run += int(gt.sum())
        eq_run += int(eq.sum())
    assert gt_run == above and eq_run >= need_eq
    cand = np.sort(cand)[::-1]                    # descending words: rank descending, then column ascending
    return (np.uint64(0xFFFFFFFF) - (cand & np.uint64(0xFFFFFFFF))).astype(np.int64)


def model_rows():
    rng = np.random.RandomState(5)
    rows = [("all zero", np.zeros(5000, np.int64), 9), ("all equal", np.full(3001, 77, np.int64), 9),
            ("strictly increasing", np.arange(4100, dtype=np.int64), 13), ("strictly decreasing", np.arange(4100, dtype=np.int64)[::-1], 13),
            ("one element", np.array([3], np.int64), 4), ("16-bit ranks", rng.randint(0, 65536, 7000).astype(np.int64), 16)]
    for n, hi, bits in [(100, 4, 3), (2047, 3, 9), (2049, 501, 9), (6000, 3001, 12), (9000, 40, 9), (12345, 2, 1)]:
        rows.append(("random with heavy ties n=%d hi=%d" % (n, hi), rng.randint(0, hi, n).astype(np.int64), bits))
    sparse = np.zeros(10000, np.int64)                         # mostly zero, as unrelated peptides are
    sparse[rng.randint(0, 10000, 30)] = rng.randint(1, 500, 30)
    rows.append(("mostly zero", sparse, 9))
    return rows


@pytest.mark.parametrize("name,row,bits", model_rows(), ids=[r[0] for r in model_rows()])
def test_model_of_the_selection_equals_stable_argsort(name, row, bits):
    assert int(row.max()) < (1 << bits)
    n = len(row)
    for top in sorted({1, 2, 10, min(n, 1024), min(n, 1000), max(1, min(n, 1024) - 1)}):
        if top > n:
            continue
        want = np.argsort(-row, kind="stable")[:top]
        assert np.array_equal(model_topk(row, top, bits), want), (name, top)
