"""CPU tests of the exact Jaccard index for sequences of up to 1024 shingle positions: the new symbols and Python names, every validation path
of the _long entry points -- status, text and order, all before a device is needed -- the short calls' unchanged limit, and the code / value-rank
contract: every (intersection, union) the limits allow lies in the domain of nw_value_ranks(S), S the largest shingle count, and the value
behind its rank is Python's divide of the two integers, bit for bit.  No compute calls here."""
import ctypes
import inspect

import numpy as np
import pytest

import oracle_lib as O

SYMBOLS = ["da_similarity_jaccard_long", "da_similarity_jaccard_cross_long", "da_similarity_jaccard_cross_topk_long", "da_similarity_jaccard_knn_long",
           "da_similarity_jaccard_edges_long_begin", "da_similarity_jaccard_cross_edges_long_begin", "da_similarity_jaccard_stats_long",
           "da_jaccard_sets_long_ld", "da_dev_jaccard_sets_long", "da_dev_jaccard_rect_long"]
OK, EMPTY, BAD_K, NO_DEVICE, UNSUPPORTED, BAD_ARG = 0, 1, 2, 8, 10, 11
K_LIMIT = "the exact Jaccard index packs a shingle into one 64-bit key: k <= 8 (got 9)"
SECOND = "a nearest neighbour needs a second sequence"
TWO = "the threshold is a quantile of the strict upper triangle: need >= 2 sequences"
TWO_STATS = "the statistics are over the strict upper triangle: need >= 2 sequences"
THRESH_P = "thresh_p must be in [0, 1]"


def too_long(i, positions=1025):
    return "sequence %d has %d shingle positions: the exact Jaccard index takes at most 1024 (length - k + 1 <= 1024)" % (i, positions)


def too_long_short(i):
    return "sequence %d has 128 shingle positions: the exact Jaccard index takes at most 127 (length - k + 1 <= 127)" % i


@pytest.fixture(scope="module")
def lib(built):
    from dynaalign_amd import _capi
    return _capi.load()


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    return dynaalign_amd


# ---- symbols and mirror --------------------------------------------------------------------------------------------------------------------

def test_header_library_and_signatures_agree_on_the_long_jaccard_symbols(lib):
    from dynaalign_amd import _capi
    declared = _capi.header_symbols()
    for name in SYMBOLS:
        assert name in declared and name in _capi.SIGNATURES and hasattr(lib, name), name
    assert sorted(_capi.SIGNATURES) == declared
    short = {"da_similarity_jaccard_long": "da_similarity_jaccard", "da_similarity_jaccard_cross_long": "da_similarity_jaccard_cross",
             "da_similarity_jaccard_cross_topk_long": "da_similarity_jaccard_cross_topk", "da_similarity_jaccard_knn_long": "da_similarity_jaccard_knn",
             "da_similarity_jaccard_edges_long_begin": "da_similarity_jaccard_edges_begin", "da_dev_jaccard_sets_long": "da_dev_jaccard_sets",
             "da_dev_jaccard_rect_long": "da_dev_jaccard_rect", "da_jaccard_sets_long_ld": "da_dev_jaccard_sets_ld"}
    for long_name, short_name in short.items():                                     # a _long sibling takes its short call's arguments
        assert _capi.SIGNATURES[long_name] == _capi.SIGNATURES[short_name], long_name
    assert lib.da_abi_version() == 2                                                  # entry points only: the version stays


def test_python_mirror_exports(da):
    from dynaalign_amd import device
    params = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]      # noqa: E731
    for name in ("similarityJaccard", "similarityJaccard_cross", "similarityJaccard_cross_topk", "similarityJaccard_knn", "similarityJaccard_knn_edges",
                 "similarityJaccard_edges"):
        assert name + "_long" in da.__all__ and callable(getattr(da, name + "_long")), name
        assert params(getattr(da, name + "_long")) == params(getattr(da, name)), name
    none = inspect.Parameter.empty
    for name in ("similarityJaccard_cross_edges_long", "similarityJaccard_stats_long"):
        assert name in da.__all__ and callable(getattr(da, name)), name
    assert params(da.similarityJaccard_cross_edges_long) == [("x", none), ("y", none), ("k", 4), ("thresh_p", 0.8), ("threshold", None)]
    assert params(da.similarityJaccard_stats_long) == [("sequences", none), ("k", 4)]
    assert params(device.jaccard_sets_long) == params(device.jaccard_sets)
    assert params(device.jaccard_rect_long) == params(device.jaccard_rect)
    assert params(da.jaccard_dense) == [("sequences", none), ("k", none), ("y", None)]      # the definition has no limit to lift


# ---- validation: status, text, order -- no device ------------------------------------------------------------------------------------------

def err(lib, rc):
    return rc, lib.da_last_error().decode("latin-1") if rc else ""


def p_(a):
    return None if a is None else a.ctypes.data


def square(lib, seqs, k, res=True, off=True, out=True, entry="da_similarity_jaccard_long"):
    r, o = O.pack(seqs)
    buf = np.full(max(len(seqs), 1) ** 2, -7.0)
    return err(lib, getattr(lib, entry)(p_(r if res else None), p_(o if off else None), len(seqs), k, p_(buf if out else None)))


def knn(lib, seqs, k, top, idx=True, entry="da_similarity_jaccard_knn_long"):
    r, o = O.pack(seqs)
    cnt = max(len(seqs), 1) * max(top, 1)
    ib, vb = np.full(cnt, -7, np.int32), np.full(cnt, -7.0)
    return err(lib, getattr(lib, entry)(r.ctypes.data, o.ctypes.data, len(seqs), k, top, p_(ib if idx else None), vb.ctypes.data))


def edges(lib, seqs, k, p, entry="da_similarity_jaccard_edges_long_begin"):
    r, o = O.pack(seqs)
    thr, cnt = np.zeros(1), np.zeros(1, np.int64)
    h = ctypes.c_void_p()
    rc = getattr(lib, entry)(r.ctypes.data, o.ctypes.data, len(seqs), k, p, ctypes.addressof(h), thr.ctypes.data, cnt.ctypes.data)
    if rc == OK:
        lib.da_edges_free(h)
    else:
        assert h.value is None
    return err(lib, rc)


def stats(lib, seqs, k, out=True):
    from dynaalign_amd import _capi
    r, o = O.pack(seqs)
    s = _capi.DaSimilarityStats()
    return err(lib, lib.da_similarity_jaccard_stats_long(r.ctypes.data, o.ctypes.data, len(seqs), k, ctypes.addressof(s) if out else None))


def cross(lib, x, y, k, topk=None, out=True):
    xr, xo = O.pack(x)
    yr, yo = O.pack(y)
    if topk is None:
        buf = np.full(max(len(x), 1) * max(len(y), 1), -7.0)
        return err(lib, lib.da_similarity_jaccard_cross_long(xr.ctypes.data, xo.ctypes.data, len(x), yr.ctypes.data, yo.ctypes.data, len(y), k,
                                                             p_(buf if out else None), 0))
    cnt = max(len(x), 1) * max(topk, 1)
    ib, vb = np.full(cnt, -7, np.int32), np.full(cnt, -7.0)
    return err(lib, lib.da_similarity_jaccard_cross_topk_long(xr.ctypes.data, xo.ctypes.data, len(x), yr.ctypes.data, yo.ctypes.data, len(y), k, topk,
                                                              p_(ib if out else None), vb.ctypes.data))


def cross_edges(lib, x, y, k, thresh, is_q, xres=True):
    xr, xo = O.pack(x)
    yr, yo = O.pack(y)
    thr, cnt = np.zeros(1), np.zeros(1, np.int64)
    h = ctypes.c_void_p()
    rc = lib.da_similarity_jaccard_cross_edges_long_begin(p_(xr if xres else None), xo.ctypes.data, len(x), yr.ctypes.data, yo.ctypes.data, len(y), k,
                                                          thresh, is_q, ctypes.addressof(h), thr.ctypes.data, cnt.ctypes.data)
    got = err(lib, rc)
    if rc == OK:
        lib.da_edges_free(h)
    else:
        assert h.value is None
    return got + ((float(thr[0]), int(cnt[0])) if rc == OK else ())


def passes(result):
    """the validation let the call through: it ran (a device is present) or stopped at the device check, the last one"""
    return result[0] in (OK, NO_DEVICE)


LONG1032, LONG1031 = "AC" * 516, "AC" * 515 + "A"       # at k = 8: 1025 and 1024 shingle positions
TWO_SEQS = ["ACDEFGHIK", "ACDEFGHIR"]


def test_one_set_validation_order_and_texts(lib, da, kats):
    e = kats["mh_errors"]
    two = TWO_SEQS
    calls = {"square": lambda s, k: square(lib, s, k), "knn": lambda s, k: knn(lib, s, k, 1), "edges_begin": lambda s, k: edges(lib, s, k, 0.8),
             "stats": lambda s, k: stats(lib, s, k)}
    for name, call in calls.items():
        assert call([], 4) == (EMPTY, e["empty"]), name
        assert call([], 0) == (EMPTY, e["empty"]), name                            # n before k
        assert call(two, 0) == (BAD_K, e["k"]) and call(two, -1) == (BAD_K, e["k"]), name
        assert call([LONG1032], 0) == (BAD_K, e["k"]), name                        # k before the limits
        assert call(two, 9) == (UNSUPPORTED, K_LIMIT), name
        assert call(two + [LONG1032], 9) == (UNSUPPORTED, K_LIMIT), name           # k > 8 before the lengths
        assert call(two + [LONG1032], 8) == (UNSUPPORTED, too_long(3)), name
        assert call([LONG1032] + two, 8) == (UNSUPPORTED, too_long(1)), name
        assert call(two + ["A" * 1025], 1) == (UNSUPPORTED, too_long(3)), name
        assert call(two + ["A" * 2000], 4) == (UNSUPPORTED, too_long(3, 1997)), name
        assert passes(call(two + [LONG1031], 8)), name                             # 1024 shingle positions: the limit itself
        assert passes(call(["A" * 1024, "", "A"], 1)), name                        # 1024 positions at k = 1; empty and short sequences are legal
    # NULL pointers after n and k, before the offsets
    assert square(lib, two, 4, res=False)[0] == BAD_ARG and square(lib, two, 4, out=False)[0] == BAD_ARG
    assert square(lib, two, 0, res=False) == (BAD_K, e["k"])
    assert square(lib, two, 4, off=False) == (BAD_ARG, "offsets is NULL")
    assert knn(lib, two, 4, 1, idx=False)[0] == BAD_ARG
    assert stats(lib, two, 4, out=False)[0] == BAD_ARG and stats(lib, two, 0, out=False) == (BAD_K, e["k"])
    # decreasing offsets, before the limits
    r, o = O.pack(two + [LONG1032])
    o = o.copy()
    o[1], o[2] = o[2], o[1]
    buf = np.full(9, -7.0)
    assert err(lib, lib.da_similarity_jaccard_long(r.ctypes.data, o.ctypes.data, 3, 9, buf.ctypes.data)) == \
        (BAD_ARG, "offsets must be non-decreasing (sequence 1)")
    # the Python mirror raises the same
    for fn in (da.similarityJaccard_long, da.similarityJaccard_knn_long, da.similarityJaccard_knn_edges_long, da.similarityJaccard_edges_long,
               da.similarityJaccard_stats_long):
        for seqs, k, code, msg in [([], 4, EMPTY, e["empty"]), (two, 0, BAD_K, e["k"]), (two, 9, UNSUPPORTED, K_LIMIT),
                                   (two + [LONG1032], 8, UNSUPPORTED, too_long(3))]:
            with pytest.raises(da.DynaAlignError) as ei:
                fn(seqs, k)
            assert (ei.value.code, str(ei.value)) == (code, msg), (fn.__name__, k)


def test_knn_edges_and_stats_checks_follow_the_shared_ones(lib, da):
    three = ["ACDEFGHIK", "ACDEFGHIR", "ACDEFGHIW"]
    for top in (0, 1, 2000):
        assert knn(lib, ["ACDE"], 4, top) == (BAD_ARG, SECOND)                     # n = 1: no neighbour, whatever top
    for top in (0, -1, 3, 4):
        assert knn(lib, three, 4, top) == (BAD_ARG, "top must be in 1 .. n - 1 (got top = %d, n = 3)" % top)
    many = ["ACDE"] * 1030
    assert knn(lib, many, 4, 1025) == (UNSUPPORTED, "top-k per row keeps its candidates in a fixed LDS buffer: top <= 1024 (got 1025)")
    assert knn(lib, many, 4, 1030)[0] == BAD_ARG                                    # top > n - 1 before top > 1024
    assert knn(lib, three, 9, 0) == (UNSUPPORTED, K_LIMIT)                          # the shared checks first
    assert knn(lib, three + [LONG1032], 8, 0) == (UNSUPPORTED, too_long(4))
    assert passes(knn(lib, three, 4, 2))
    with pytest.raises(da.DynaAlignError) as ei:
        da.similarityJaccard_knn_long(["ACDE"], 4)
    assert (ei.value.code, str(ei.value)) == (BAD_ARG, SECOND)
    assert edges(lib, ["ACDE"], 4, 0.8) == (BAD_ARG, TWO)                          # edges with n = 1
    assert edges(lib, ["ACDE"], 4, 1.5) == (BAD_ARG, TWO)                          # ... before thresh_p
    for p in (-0.1, 1.0001, float("nan")):
        assert edges(lib, three, 4, p) == (BAD_ARG, THRESH_P)
    assert edges(lib, three, 9, 1.5) == (UNSUPPORTED, K_LIMIT)
    assert edges(lib, three + [LONG1032], 8, 1.5) == (UNSUPPORTED, too_long(4))
    assert passes(edges(lib, three, 4, 0.0)) and passes(edges(lib, three, 4, 1.0))
    r, o = O.pack(three)
    assert lib.da_similarity_jaccard_edges_long_begin(r.ctypes.data, o.ctypes.data, 3, 4, 0.8, None, None, None) == BAD_ARG
    assert stats(lib, ["ACDE"], 4) == (BAD_ARG, TWO_STATS)
    assert stats(lib, ["ACDE"], 9) == (UNSUPPORTED, K_LIMIT)                        # the shared checks first
    assert passes(stats(lib, ["", ""], 4)) and passes(stats(lib, ["", "A", "ACDEF"], 4))      # empty sets are legal here, unlike in the NW statistics


def test_two_set_validation(lib, da, kats):
    e = kats["mh_errors"]
    x, y = ["ACDEFGHIK", "ACDEFGHIR"], ["ACDEFGHIW", "ACDEFGHIK", "AC"]
    for topk in (None, 1):
        assert cross(lib, x, y, 0, topk) == (BAD_K, e["k"]) and cross(lib, [], [], -1, topk) == (BAD_K, e["k"])
        assert cross(lib, [], y, 4, topk) == (OK, "")                               # no rows: nothing to write
        assert cross(lib, x, y, 4, topk, out=False)[0] == BAD_ARG
        assert cross(lib, x, y, 9, topk) == (UNSUPPORTED, K_LIMIT)
        assert cross(lib, x + [LONG1032], y, 8, topk) == (UNSUPPORTED, too_long(3))
        assert cross(lib, x, [LONG1032] + y, 8, topk) == (UNSUPPORTED, too_long(1))
        assert cross(lib, x + [LONG1032], [LONG1032] + y, 8, topk) == (UNSUPPORTED, too_long(3))      # x before y
        assert passes(cross(lib, x, y + [LONG1031], 8, topk))
    assert cross(lib, x, [], 4) == (OK, "")                                          # an m x 0 matrix
    assert cross(lib, x, [], 4, 1) == (BAD_ARG, "top must be in 1 .. n (got top = 1, n = 0)")
    for top in (0, -1, 4):                                                          # top = 0, top = n + 1
        assert cross(lib, x, y, 4, top) == (BAD_ARG, "top must be in 1 .. n (got top = %d, n = 3)" % top)
    many = ["ACDE"] * 1030
    assert cross(lib, x, many, 4, 1025) == (UNSUPPORTED, "top-k per row keeps its candidates in a fixed LDS buffer: top <= 1024 (got 1025)")
    assert cross(lib, x, many, 9, 0) == (UNSUPPORTED, K_LIMIT)                      # the limits before top
    assert da.similarityJaccard_cross_long([], y, 4).shape == (0, 3) and da.similarityJaccard_cross_long(x, [], 4).shape == (2, 0)
    idx, val = da.similarityJaccard_cross_topk_long([], y, 4, 2)
    assert idx.shape == (0, 2) and val.shape == (0, 2)


def test_two_set_threshold_form_validation(lib, da, kats):
    e = kats["mh_errors"]
    x, y = ["ACDEFGHIK", "ACDEFGHIR"], ["ACDEFGHIW", "ACDEFGHIK", "AC"]
    nan = float("nan")
    assert cross_edges(lib, x, y, 0, 0.8, 1) == (BAD_K, e["k"]) and cross_edges(lib, [], [], -1, 0.8, 1) == (BAD_K, e["k"])
    # an empty rectangle: the threshold check, then no quantile / no edges
    for a, b in (([], y), (x, []), ([], [])):
        assert cross_edges(lib, a, b, 4, 1.5, 1) == (BAD_ARG, THRESH_P)
        assert cross_edges(lib, a, b, 4, nan, 0)[0] == BAD_ARG
        assert cross_edges(lib, a, b, 4, 0.8, 1) == (BAD_ARG, "quantile of an empty set")
        assert cross_edges(lib, a, b, 4, 0.25, 0) == (OK, "", 0.25, 0)
    assert cross_edges(lib, x, y, 4, 0.8, 1, xres=False)[0] == BAD_ARG
    assert cross_edges(lib, x, y, 9, 1.5, 1) == (UNSUPPORTED, K_LIMIT)              # the limits before the threshold
    assert cross_edges(lib, x + [LONG1032], y, 8, 1.5, 1) == (UNSUPPORTED, too_long(3))
    assert cross_edges(lib, x, [LONG1032] + y, 8, 0.8, 1) == (UNSUPPORTED, too_long(1))
    for p in (-0.1, 1.0001, nan):
        assert cross_edges(lib, x, y, 4, p, 1) == (BAD_ARG, THRESH_P)
    assert cross_edges(lib, x, y, 4, nan, 0)[0] == BAD_ARG
    assert passes(cross_edges(lib, x, y + [LONG1031], 8, 0.5, 1)) and passes(cross_edges(lib, x, y, 4, 7.0, 0))      # any absolute threshold that is a number
    xr, xo = O.pack(x)
    assert lib.da_similarity_jaccard_cross_edges_long_begin(xr.ctypes.data, xo.ctypes.data, 2, xr.ctypes.data, xo.ctypes.data, 2, 4, 0.8, 1, None, None,
                                                            None) == BAD_ARG
    with pytest.raises(da.DynaAlignError) as ei:
        da.similarityJaccard_cross_edges_long(x, [], 4)
    assert (ei.value.code, str(ei.value)) == (BAD_ARG, "quantile of an empty set")
    thr, ei_, ej, w = da.similarityJaccard_cross_edges_long([], y, 4, threshold=0.5)
    assert thr == 0.5 and len(ei_) == len(ej) == len(w) == 0


def test_the_short_calls_still_refuse_128_positions_with_their_old_text(lib, da):
    long135 = "AC" * 67 + "A"
    two = TWO_SEQS
    assert square(lib, two + [long135], 8, entry="da_similarity_jaccard") == (UNSUPPORTED, too_long_short(3))
    assert knn(lib, two + [long135], 8, 1, entry="da_similarity_jaccard_knn") == (UNSUPPORTED, too_long_short(3))
    assert edges(lib, [long135] + two, 8, 0.8, entry="da_similarity_jaccard_edges_begin") == (UNSUPPORTED, too_long_short(1))
    assert passes(square(lib, two + [long135], 8)) and passes(knn(lib, two + [long135], 8, 1))      # what the long calls are for
    with pytest.raises(da.DynaAlignError) as ei:
        da.similarityJaccard(two + [long135], 8)
    assert (ei.value.code, str(ei.value)) == (UNSUPPORTED, too_long_short(3))
    fake = 4096
    rc = lib.da_dev_jaccard_sets(fake, fake, 3, 135, 8, fake, 128, fake, None)
    assert err(lib, rc) == (UNSUPPORTED, "max_len - k + 1 = 128 shingle positions: the exact Jaccard index takes at most 127")


def test_device_layer_argument_checks(lib):
    e = lambda rc: err(lib, rc)                                                     # noqa: E731
    assert [lib.da_jaccard_sets_long_ld(ml, k) for ml, k in [(0, 4), (3, 4), (4, 4), (12, 2), (20, 4), (21, 4), (134, 8), (566, 4), (1024, 1), (1031, 8), (5, 0)]] == \
        [4, 4, 4, 12, 20, 20, 128, 564, 1024, 1024, 0]
    fake = 4096                                                                     # never dereferenced: every call below is refused first
    sets = lambda n, ml, k, keys=fake, ld=1024, cnt=fake, res=fake: e(lib.da_dev_jaccard_sets_long(res, fake, n, ml, k, keys, ld, cnt, None))      # noqa: E731
    assert sets(0, 20, 4)[0] == EMPTY and sets(3, 20, 0)[0] == BAD_K and sets(0, 20, 0)[0] == EMPTY
    assert sets(3, 20, 4, keys=None)[0] == BAD_ARG and sets(3, 20, 4, cnt=None)[0] == BAD_ARG and sets(3, 20, 4, res=None)[0] == BAD_ARG
    assert sets(3, 20, 9) == (UNSUPPORTED, K_LIMIT)
    assert sets(3, 1032, 8) == (UNSUPPORTED, "max_len - k + 1 = 1025 shingle positions: the exact Jaccard index takes at most 1024")
    assert sets(3, -1, 4)[0] == BAD_ARG
    assert sets(3, 600, 4, ld=596)[0] == BAD_ARG and sets(3, 20, 4, ld=1025)[0] == BAD_ARG      # ld_keys too small / beyond the 1024 slots
    assert sets(3, 20, 4, keys=fake + 2)[0] == BAD_ARG and sets(3, 20, 5, keys=fake + 4)[0] == BAD_ARG      # keys aligned to their size
    assert sets(3, 20, 4, cnt=fake + 1)[0] == BAD_ARG                              # uint16 counts
    rect = lambda n=10, ld_keys=600, k=4, r=(0, 10), c=(0, 10), kind=2, out=fake, ld=10, keys=fake, cnt=fake: e(      # noqa: E731
        lib.da_dev_jaccard_rect_long(keys, cnt, n, ld_keys, k, r[0], r[1], c[0], c[1], kind, out, ld, None))
    assert rect(k=0)[0] == BAD_K and rect(k=9) == (UNSUPPORTED, K_LIMIT)
    assert rect(keys=None)[0] == BAD_ARG and rect(out=None)[0] == BAD_ARG and rect(cnt=None)[0] == BAD_ARG and rect(n=-1)[0] == BAD_ARG
    assert rect(r=(-1, 3))[0] == BAD_ARG and rect(r=(4, 3))[0] == BAD_ARG and rect(r=(0, 11))[0] == BAD_ARG
    assert rect(c=(-1, 3))[0] == BAD_ARG and rect(c=(4, 3))[0] == BAD_ARG and rect(c=(0, 11))[0] == BAD_ARG
    assert rect(ld=9)[0] == BAD_ARG and rect(ld_keys=0)[0] == BAD_ARG and rect(ld_keys=1025)[0] == BAD_ARG
    assert rect(kind=1) == (BAD_ARG, "bad output kind") and rect(kind=3) == (BAD_ARG, "bad output kind")      # PACK32 or F64, no uint16 code
    assert rect(out=fake + 2)[0] == BAD_ARG and rect(kind=0, out=fake + 4)[0] == BAD_ARG      # naturally aligned output
    assert rect(r=(3, 3)) == (OK, "") and rect(c=(10, 10), ld=0) == (OK, "")       # an empty rectangle is DA_OK, before any launch
    assert rect(kind=0, r=(3, 3)) == (OK, "")


# ---- codes, values and the value ranks -----------------------------------------------------------------------------------------------------

def domain(S):
    """every (intersection, union) two sets of at most S shingles can have: ca, cb <= S share i <= min(ca, cb), union = ca + cb - i"""
    return {(i, ca + cb - i) for ca in range(S + 1) for cb in range(ca, S + 1) for i in range(ca + 1)} - {(0, 0)}


@pytest.mark.parametrize("S", [1, 2, 40])
def test_every_possible_code_has_a_value_rank_with_its_value(da, S):
    values, rank = da.nw_value_ranks(S)
    assert rank.shape == (2 * S + 1, S + 1)
    pairs = domain(S)
    assert all(1 <= u <= 2 * S and 0 <= i <= min(u, S) for i, u in pairs)            # inside the table
    assert (1, 1) in pairs and (S, S) in pairs and (0, 2 * S) in pairs               # two empty sets are coded 1 << 16 | 1: the value 1.0
    for i in range(S + 1):                                                           # and the whole of the stated domain, reachable or not
        for u in range(max(i, 1), 2 * S + 1):
            v = values[rank[u, i]]
            assert np.float64(v).view(np.uint64) == np.float64(i / u).view(np.uint64), (i, u)
    by_value = {}
    for i, u in pairs:
        by_value.setdefault(i / u, set()).add(int(rank[u, i]))
    assert all(len(r) == 1 for r in by_value.values())                              # equal values, equal ranks
    order = sorted(by_value)
    got = [next(iter(by_value[v])) for v in order]
    assert got == sorted(got) and len(set(got)) == len(got) and got[0] == 0         # a larger value, a larger rank; 0.0 is rank 0
    assert np.all(np.diff(values) > 0)


def test_value_ranks_at_1024_shingles(da):
    S = 1024
    values, rank = da.nw_value_ranks(S)
    rng = np.random.RandomState(5)
    pairs = [(1024, 1024), (0, 2048), (1, 2047), (1, 1), (0, 1), (1024, 2048), (512, 1024), (1023, 1025), (341, 1023), (682, 2046)]
    while len(pairs) < 400:
        ca, cb = rng.randint(0, S + 1, 2)
        i = rng.randint(0, min(ca, cb) + 1)
        if ca + cb - i:
            pairs.append((int(i), int(ca + cb - i)))
    for i, u in pairs:
        assert 1 <= u <= 2 * S and i <= min(u, S)
        assert np.float64(values[rank[u, i]]).view(np.uint64) == np.float64(i / u).view(np.uint64), (i, u)
    assert rank[2048, 1024] == rank[1024, 512] == rank[2, 1] and rank[1023, 341] == rank[2046, 682] == rank[3, 1]
    assert rank[2048, 0] == 0 and rank[1024, 1024] == rank[1, 1] == len(values) - 1
    assert rank[2048, 1] == 1 and rank[2047, 1] == 2                                 # the two smallest positive values: 1/2048 < 1/2047
