"""CPU tests of the Levenshtein similarity: lev_dense / lev_counts (the package's statement of the definition) against hand-written cases and
against a cell-by-cell DP written here, the new symbols, every validation path of the C ABI -- status, text and order, all before a device is
needed -- the code / rank-table contract (every code the limit allows lies in the domain of da_nw_code_ranks(127) and its value is the divide of
its two integers), and the device layer's refusal of host tensors.  No compute calls here."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import oracle_lib as O

SYMBOLS = ["da_similarity_lev", "da_similarity_lev_cross", "da_similarity_lev_cross_topk", "da_similarity_lev_knn", "da_similarity_lev_edges",
           "da_similarity_lev_edges_begin", "da_similarity_lev_cross_edges_begin", "da_dev_lev_masks_bytes", "da_dev_lev_masks", "da_dev_lev_rect"]
OK, EMPTY, NO_DEVICE, UNSUPPORTED, BAD_ARG = 0, 1, 8, 10, 11
SECOND = "a nearest neighbour needs a second sequence"
TWO = "the threshold is a quantile of the strict upper triangle: need >= 2 sequences"
TOP_LDS = "top-k per row keeps its candidates in a fixed LDS buffer: top <= 1024 (got 1025)"
LONG128, LONG127 = "AC" * 64, "AC" * 63 + "A"


def too_long(i):
    return "sequence %d is 128 bytes long: the Levenshtein similarity takes sequences of at most 127 bytes" % i


@pytest.fixture(scope="module")
def lib(built):
    from dynaalign_amd import _capi
    return _capi.load()


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    return dynaalign_amd


def distance(a, b):
    """the textbook recurrence, one cell at a time"""
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1]))
        prev = cur
    return prev[len(b)]


# ---- the definition ------------------------------------------------------------------------------------------------------------------------

def test_lev_dense_hand_written_cases(da):
    num, den = da.lev_counts(["kitten", "sitting"])
    assert num.dtype == den.dtype == np.int64 and num.shape == (2, 2)
    assert den[0, 1] == den[1, 0] == 7 and num[0, 1] == num[1, 0] == 7 - 3        # kitten / sitting: 3 edits
    S = da.lev_dense(["kitten", "sitting"])
    assert S.dtype == np.float64 and S[0, 1] == S[1, 0] == 4 / 7 and S[0, 0] == S[1, 1] == 1.0
    S = da.lev_dense(["", "", "A", "AB"])
    assert np.array_equal(S, np.array([[1.0, 1, 0, 0], [1, 1, 0, 0], [0, 0, 1, 0.5], [0, 0, 0.5, 1]]))      # "" / "" -> 1.0, "" / "A" -> 0.0
    num, den = da.lev_counts(["", "A"])
    assert (num[0, 0], den[0, 0], num[0, 1], den[0, 1]) == (0, 0, 0, 1)
    # insert, delete, substitute and a shift by one residue
    num, den = da.lev_counts(["ACDEFGHIKL"], ["ACDEFGHIKL", "ACDEFGHIK", "ACDEFGHIKLM", "ACDEFGHIKW", "CDEFGHIKLM", "LKIHGFEDCA"])
    assert den[0].tolist() == [10, 10, 11, 10, 10, 10] and (den - num)[0].tolist() == [0, 1, 1, 1, 2, 10]
    # bytes >= 0x80, str (latin-1) and bytes alike; 0x00 and 0xFF are bytes like any other
    a, b = b"AC\xff\x00\x80DE", "AC\xff\x00\x81DE"
    num, den = da.lev_counts([a, b, b"\xff" * 7, "\x80\x81\x82"])
    assert (den - num)[0].tolist() == [0, 1, 6, 6] and den[0].tolist() == [7, 7, 7, 7]
    assert np.array_equal(da.lev_dense([a, b]), da.lev_dense([a.decode("latin-1"), b.encode("latin-1")]))
    # the two-set form is the block of the square one
    x, y = ["ABCDEF", "", "QRS"], ["BCDEFG", "A", "ABCDEF", "QRSQRS", ""]
    assert np.array_equal(da.lev_dense(x, y), da.lev_dense(x + y)[:3, 3:])
    assert da.lev_dense(x, y).shape == (3, 5) and da.lev_dense([], y).shape == (0, 5)


def test_lev_counts_against_the_cell_by_cell_dp(da):
    rng = np.random.RandomState(8)
    alphabet = [bytes([c]) for c in b"ACD"] + [b"\xff", b"\x00", b"\x80"]
    seqs = [b"".join(alphabet[t] for t in rng.randint(0, len(alphabet), rng.randint(0, 14))) for _ in range(60)]
    seqs += [seqs[3], seqs[4][1:], seqs[5] + b"A"]
    num, den = da.lev_counts(seqs)
    want_d = np.array([[distance(a, b) for b in seqs] for a in seqs])
    want_l = np.array([[max(len(a), len(b)) for b in seqs] for a in seqs])
    assert np.array_equal(den, want_l) and np.array_equal(den - num, want_d)
    S = da.lev_dense(seqs)
    want = np.array([[((ln - d) / ln) if ln else 1.0 for d, ln in zip(rd, rl)] for rd, rl in zip(want_d, want_l)])
    assert np.array_equal(S.view(np.uint64), want.view(np.uint64))
    assert np.array_equal(S, S.T) and np.all(np.diag(S) == 1.0) and not np.isnan(S).any()
    # the input has something of everything: two empty strings, one empty string, identical strings off the diagonal, partial matches
    assert (want_l == 0).sum() > 0 and ((want_d == want_l) & (want_l > 0)).sum() > 0 and (S == 1.0).sum() > len(seqs) and len(np.unique(S)) > 20


# ---- symbols and mirror --------------------------------------------------------------------------------------------------------------------

def test_header_library_and_signatures_agree_on_the_lev_symbols(lib):
    from dynaalign_amd import _capi
    declared = _capi.header_symbols()
    for name in SYMBOLS:
        assert name in declared and name in _capi.SIGNATURES and hasattr(lib, name), name
    assert sorted(_capi.SIGNATURES) == declared
    assert lib.da_abi_version() == 2                                                  # entry points only: the version stays


def test_python_mirror_exports(da):
    from dynaalign_amd import device
    for name in ("lev_dense", "lev_counts", "similarityLev", "similarityLev_cross", "similarityLev_cross_topk", "similarityLev_knn",
                 "similarityLev_knn_edges", "similarityLev_edges", "similarityLev_cross_edges"):
        assert name in da.__all__ and callable(getattr(da, name)), name
    params = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]      # noqa: E731
    none = inspect.Parameter.empty
    assert params(da.lev_dense) == params(da.lev_counts) == [("sequences", none), ("y", None)]
    assert params(da.similarityLev) == [("sequences", none)]
    assert params(da.similarityLev_cross) == [("x", none), ("y", none)]
    assert params(da.similarityLev_cross_topk) == [("x", none), ("y", none), ("top", 10)]
    assert params(da.similarityLev_knn) == [("sequences", none), ("top", 10)]
    assert params(da.similarityLev_knn_edges) == [("sequences", none), ("top", 10), ("mode", "union")]
    assert params(da.similarityLev_edges) == [("sequences", none), ("thresh_p", 0.8)]
    assert params(da.similarityLev_cross_edges) == [("x", none), ("y", none), ("thresh_p", 0.8), ("threshold", None)]
    assert inspect.signature(da.similarityLev_cross_edges).parameters["threshold"].kind is inspect.Parameter.KEYWORD_ONLY
    assert [p for p, _ in params(device.lev_masks)] == ["ds", "class_map"]
    assert [p for p, _ in params(device.lev_rect)] == ["masks", "row_begin", "row_end", "col_begin", "col_end", "kind", "out"]


# ---- validation: status, text, order -- no device ------------------------------------------------------------------------------------------

def err(lib, rc):
    return rc, lib.da_last_error().decode("latin-1") if rc else ""


def p_(a):
    return None if a is None else a.ctypes.data


def square(lib, seqs, res=True, off=True, out=True):
    r, o = O.pack(seqs)
    buf = np.full(max(len(seqs), 1) ** 2, -7.0)
    return err(lib, lib.da_similarity_lev(p_(r if res else None), p_(o if off else None), len(seqs), p_(buf if out else None)))


def knn(lib, seqs, top, idx=True):
    r, o = O.pack(seqs)
    cnt = max(len(seqs), 1) * max(top, 1)
    ib, vb = np.full(cnt, -7, np.int32), np.full(cnt, -7.0)
    return err(lib, lib.da_similarity_lev_knn(r.ctypes.data, o.ctypes.data, len(seqs), top, p_(ib if idx else None), vb.ctypes.data))


def edges(lib, seqs, p, begin=False):
    r, o = O.pack(seqs)
    thr, cnt = np.zeros(1), np.zeros(1, np.int64)
    if begin:
        h = ctypes.c_void_p()
        rc = lib.da_similarity_lev_edges_begin(r.ctypes.data, o.ctypes.data, len(seqs), p, ctypes.addressof(h), thr.ctypes.data, cnt.ctypes.data)
        if rc == OK:
            lib.da_edges_free(h)
        else:
            assert h.value is None
        return err(lib, rc)
    return err(lib, lib.da_similarity_lev_edges(r.ctypes.data, o.ctypes.data, len(seqs), p, thr.ctypes.data, cnt.ctypes.data, 0, None, None, None))


def cross(lib, x, y, topk=None, out=True):
    xr, xo = O.pack(x)
    yr, yo = O.pack(y)
    if topk is None:
        buf = np.full(max(len(x), 1) * max(len(y), 1), -7.0)
        return err(lib, lib.da_similarity_lev_cross(xr.ctypes.data, xo.ctypes.data, len(x), yr.ctypes.data, yo.ctypes.data, len(y),
                                                    p_(buf if out else None), 0))
    cnt = max(len(x), 1) * max(topk, 1)
    ib, vb = np.full(cnt, -7, np.int32), np.full(cnt, -7.0)
    return err(lib, lib.da_similarity_lev_cross_topk(xr.ctypes.data, xo.ctypes.data, len(x), yr.ctypes.data, yo.ctypes.data, len(y), topk,
                                                     p_(ib if out else None), vb.ctypes.data))


def cross_edges(lib, x, y, thresh, is_q, x_res=True):
    """-> (status, text, threshold, edges)"""
    xr, xo = O.pack(x)
    yr, yo = O.pack(y)
    thr, cnt = np.full(1, -7.0), np.full(1, -7, np.int64)
    h = ctypes.c_void_p()
    rc = lib.da_similarity_lev_cross_edges_begin(p_(xr if x_res else None), xo.ctypes.data, len(x), yr.ctypes.data, yo.ctypes.data, len(y), thresh,
                                                 is_q, ctypes.addressof(h), thr.ctypes.data, cnt.ctypes.data)
    if rc == OK:
        lib.da_edges_free(h)
    else:
        assert h.value is None
    return err(lib, rc) + (thr[0], cnt[0])


def passes(result):
    """the validation let the call through: it ran (a device is present) or stopped at the device check, the last one"""
    return result[0] in (OK, NO_DEVICE)


def test_one_set_validation_order_and_texts(lib, da, kats):
    empty = kats["mh_errors"]["empty"]
    two = ["ACDEFGHIK", "ACDEFGHIR"]
    calls = {"square": lambda s: square(lib, s), "knn": lambda s: knn(lib, s, 1), "edges": lambda s: edges(lib, s, 0.8),
             "edges_begin": lambda s: edges(lib, s, 0.8, begin=True)}
    for name, call in calls.items():
        assert call([]) == (EMPTY, empty), name
        assert call(two + [LONG128]) == (UNSUPPORTED, too_long(3)), name
        assert call([LONG128] + two) == (UNSUPPORTED, too_long(1)), name
        assert passes(call(two + [LONG127])), name                                   # 127 bytes: the limit itself
        assert passes(call(["", "", "A", "\x00\xff\x80"])), name                     # empty strings and any byte value are legal
    # NULL pointers after n, before the offsets
    assert square(lib, two, res=False)[0] == BAD_ARG and square(lib, two, out=False)[0] == BAD_ARG
    assert square(lib, [], res=False) == (EMPTY, empty)
    assert square(lib, two, off=False) == (BAD_ARG, "offsets is NULL")
    assert square(lib, two + [LONG128], res=False)[0] == BAD_ARG                      # NULL before the lengths
    assert knn(lib, two, 1, idx=False)[0] == BAD_ARG
    # decreasing offsets, before the lengths
    r, o = O.pack(two + [LONG128])
    o = o.copy()
    o[1], o[2] = o[2], o[1]
    buf = np.full(9, -7.0)
    assert err(lib, lib.da_similarity_lev(r.ctypes.data, o.ctypes.data, 3, buf.ctypes.data)) == (BAD_ARG, "offsets must be non-decreasing (sequence 1)")
    # the Python mirror raises the same
    for fn in (da.similarityLev, da.similarityLev_knn, da.similarityLev_knn_edges, da.similarityLev_edges):
        for seqs, code, msg in [([], EMPTY, empty), (two + [LONG128], UNSUPPORTED, too_long(3))]:
            with pytest.raises(da.DynaAlignError) as ei:
                fn(seqs)
            assert (ei.value.code, str(ei.value)) == (code, msg), fn.__name__


def test_knn_and_edges_checks_follow_the_shared_ones(lib, da):
    three = ["ACDEFGHIK", "ACDEFGHIR", "ACDEFGHIW"]
    for top in (0, 1, 2000):
        assert knn(lib, ["ACDE"], top) == (BAD_ARG, SECOND)                         # n = 1: no neighbour, whatever top
    for top in (0, -1, 3, 4):
        assert knn(lib, three, top) == (BAD_ARG, "top must be in 1 .. n - 1 (got top = %d, n = 3)" % top)
    many = ["ACDE"] * 1030
    assert knn(lib, many, 1025) == (UNSUPPORTED, TOP_LDS)
    assert knn(lib, many, 1030)[0] == BAD_ARG                                        # top > n - 1 before top > 1024
    assert knn(lib, three + [LONG128], 0) == (UNSUPPORTED, too_long(4))              # the shared checks first
    assert passes(knn(lib, three, 2))
    with pytest.raises(da.DynaAlignError) as ei:
        da.similarityLev_knn(["ACDE"])
    assert (ei.value.code, str(ei.value)) == (BAD_ARG, SECOND)
    for begin in (False, True):
        assert edges(lib, ["ACDE"], 0.8, begin) == (BAD_ARG, TWO)                   # edges with n = 1
        assert edges(lib, ["ACDE"], 1.5, begin) == (BAD_ARG, TWO)                   # ... before thresh_p
        for p in (-0.1, 1.0001, float("nan")):
            assert edges(lib, three, p, begin) == (BAD_ARG, "thresh_p must be in [0, 1]")
        assert edges(lib, three + [LONG128], 1.5, begin) == (UNSUPPORTED, too_long(4))
        assert passes(edges(lib, three, 0.0, begin)) and passes(edges(lib, three, 1.0, begin))
    r, o = O.pack(three)
    assert lib.da_similarity_lev_edges(r.ctypes.data, o.ctypes.data, 3, 0.8, None, None, 0, None, None, None) == BAD_ARG
    assert lib.da_similarity_lev_edges_begin(r.ctypes.data, o.ctypes.data, 3, 0.8, None, None, None) == BAD_ARG


def test_two_set_validation(lib, da):
    x, y = ["ACDEFGHIK", "ACDEFGHIR"], ["ACDEFGHIW", "ACDEFGHIK", "AC"]
    for topk in (None, 1):
        assert cross(lib, [], y, topk) == (OK, "")                                   # no rows: nothing to write
        assert cross(lib, [], y + [LONG128], topk) == (OK, "")                       # ... before anything is looked at
        assert cross(lib, x, y, topk, out=False)[0] == BAD_ARG
        assert cross(lib, x + [LONG128], y, topk, out=False)[0] == BAD_ARG           # NULL before the lengths
        assert cross(lib, x + [LONG128], y, topk) == (UNSUPPORTED, too_long(3))
        assert cross(lib, x, [LONG128] + y, topk) == (UNSUPPORTED, too_long(1))
        assert cross(lib, x + [LONG128], [LONG128] + y, topk) == (UNSUPPORTED, too_long(3))      # x before y
        assert passes(cross(lib, x, y + [LONG127, ""], topk))
    assert cross(lib, x, []) == (OK, "")                                              # an m x 0 matrix
    assert cross(lib, x, [], 1) == (BAD_ARG, "top must be in 1 .. n (got top = 1, n = 0)")
    for top in (0, -1, 4):                                                           # top = 0, top = n + 1
        assert cross(lib, x, y, top) == (BAD_ARG, "top must be in 1 .. n (got top = %d, n = 3)" % top)
    many = ["ACDE"] * 1030
    assert cross(lib, x, many, 1025) == (UNSUPPORTED, TOP_LDS)
    assert cross(lib, x + [LONG128], many, 0) == (UNSUPPORTED, too_long(3))          # the lengths before top
    assert da.similarityLev_cross([], y).shape == (0, 3) and da.similarityLev_cross(x, []).shape == (2, 0)
    idx, val = da.similarityLev_cross_topk([], y, 2)
    assert idx.shape == (0, 2) and val.shape == (0, 2)


def test_cross_edges_validation(lib, da):
    x, y = ["ACDEFGHIK", "ACDEFGHIR"], ["ACDEFGHIW", "ACDEFGHIK", "AC"]
    nan = float("nan")
    # an empty rectangle: no edges in the absolute form, no quantile; the threshold argument is checked first
    for ex, ey in (([], y), (x, []), ([], [])):
        assert cross_edges(lib, ex, ey, 0.5, 0) == (OK, "", 0.5, 0)
        assert cross_edges(lib, ex, ey, 0.5, 1)[:2] == (BAD_ARG, "quantile of an empty set")
        assert cross_edges(lib, ex, ey, 1.5, 1)[:2] == (BAD_ARG, "thresh_p must be in [0, 1]")
        assert cross_edges(lib, ex, ey, nan, 0)[:2] == (BAD_ARG, "the threshold must not be NaN")
    assert cross_edges(lib, [], y + [LONG128], 0.5, 0)[:2] == (OK, "")
    assert cross_edges(lib, x, y, 0.5, 0, x_res=False)[0] == BAD_ARG
    assert cross_edges(lib, x + [LONG128], y, nan, 0)[:2] == (UNSUPPORTED, too_long(3))          # the lengths before thresh
    assert cross_edges(lib, x, y + [LONG128], 1.5, 1)[:2] == (UNSUPPORTED, too_long(4))
    assert cross_edges(lib, x + [LONG128], [LONG128] + y, 0.5, 0)[:2] == (UNSUPPORTED, too_long(3))      # x before y
    for p in (-0.1, 1.0001, nan):
        assert cross_edges(lib, x, y, p, 1)[:2] == (BAD_ARG, "thresh_p must be in [0, 1]")
    assert cross_edges(lib, x, y, nan, 0)[:2] == (BAD_ARG, "the threshold must not be NaN")
    assert passes(cross_edges(lib, x, y, 2.0, 0)) and passes(cross_edges(lib, x, y, -1.0, 0)) and passes(cross_edges(lib, x, y + [LONG127], 0.8, 1))
    xr, xo = O.pack(x)
    yr, yo = O.pack(y)
    assert lib.da_similarity_lev_cross_edges_begin(xr.ctypes.data, xo.ctypes.data, 2, yr.ctypes.data, yo.ctypes.data, 3, 0.5, 0, None, None, None) == BAD_ARG
    thr, ei, ej, w = da.similarityLev_cross_edges([], y, threshold=0.5)
    assert thr == 0.5 and len(ei) == len(ej) == len(w) == 0
    with pytest.raises(da.DynaAlignError) as e:
        da.similarityLev_cross_edges(x + [LONG128], y)
    assert (e.value.code, str(e.value)) == (UNSUPPORTED, too_long(3))


def test_device_layer_argument_checks(lib):
    e = lambda rc: err(lib, rc)                                                     # noqa: E731
    # peq words + text rows of max_len rounded up to 4 (at least 4) + lengths, in the word shape max_len chooses
    sizes = [((10, 0, 1), 10 * 4 + 10 * 4 + 10), ((10, 20, 20), 10 * 20 * 4 + 10 * 20 + 10), ((10, 32, 3), 10 * 3 * 4 + 10 * 32 + 10),
             ((10, 33, 3), 10 * 3 * 8 + 10 * 36 + 10), ((10, 64, 256), 10 * 256 * 8 + 10 * 64 + 10), ((10, 65, 2), 10 * 2 * 16 + 10 * 68 + 10),
             ((10, 127, 256), 10 * 256 * 16 + 10 * 128 + 10), ((0, 20, 20), 0)]
    for args, want in sizes:
        assert lib.da_dev_lev_masks_bytes(*args) == want, args
    for args in [(10, 128, 20), (10, -1, 20), (-1, 20, 20), (10, 20, 0), (10, 20, 257)]:
        assert lib.da_dev_lev_masks_bytes(*args) == 0, args
    fake = 4096                                                                     # never dereferenced: every call below is refused first
    ident = np.arange(256, dtype=np.uint8)
    low = (ident % 20).astype(np.uint8)
    masks = lambda n=3, ml=20, cmap=low, c=20, buf=fake, nbytes=1 << 20, res=fake: e(      # noqa: E731
        lib.da_dev_lev_masks(res, fake, n, ml, p_(cmap), c, buf, nbytes, None))
    assert masks(n=0)[0] == EMPTY and masks(n=-1)[0] == EMPTY
    assert masks(res=None)[0] == BAD_ARG and masks(buf=None)[0] == BAD_ARG and masks(cmap=None)[0] == BAD_ARG
    assert masks(ml=-1)[0] == BAD_ARG
    assert masks(ml=128) == (UNSUPPORTED, "max_len = 128: the Levenshtein similarity takes sequences of at most 127 bytes")
    assert masks(c=0)[0] == BAD_ARG and masks(c=257)[0] == BAD_ARG
    assert masks(cmap=ident, c=255) == (BAD_ARG, "class_map[255] = 255 is no class id below n_classes = 255")
    assert masks(buf=fake + 4)[0] == BAD_ARG                                         # 8-byte aligned
    assert masks(nbytes=lib.da_dev_lev_masks_bytes(3, 20, 20) - 1)[0] == BAD_ARG     # too small
    rect = lambda n=10, ml=20, c=20, r=(0, 10), cc=(0, 10), kind=1, out=fake, ld=10, buf=fake: e(      # noqa: E731
        lib.da_dev_lev_rect(buf, n, ml, c, r[0], r[1], cc[0], cc[1], kind, out, ld, None))
    assert rect(buf=None)[0] == BAD_ARG and rect(out=None)[0] == BAD_ARG and rect(n=-1)[0] == BAD_ARG and rect(ml=-1)[0] == BAD_ARG
    assert rect(ml=128)[0] == UNSUPPORTED and rect(c=0)[0] == BAD_ARG and rect(c=257)[0] == BAD_ARG
    assert rect(r=(-1, 3))[0] == BAD_ARG and rect(r=(4, 3))[0] == BAD_ARG and rect(r=(0, 11))[0] == BAD_ARG
    assert rect(cc=(-1, 3))[0] == BAD_ARG and rect(cc=(4, 3))[0] == BAD_ARG and rect(cc=(0, 11))[0] == BAD_ARG
    assert rect(ld=9)[0] == BAD_ARG and rect(kind=2)[0] == BAD_ARG and rect(buf=fake + 4)[0] == BAD_ARG
    assert rect(out=fake + 1)[0] == BAD_ARG and rect(kind=0, out=fake + 4)[0] == BAD_ARG      # naturally aligned output
    assert rect(r=(3, 3)) == (OK, "") and rect(cc=(10, 10), ld=0) == (OK, "")       # an empty rectangle is DA_OK, before any launch


def test_device_front_end_refuses_host_tensors(da):
    from dynaalign_amd import _capi, device
    text = "%s must live in HBM (dynaalign_amd has no CPU path)"
    ds = device.DeviceSequences(np.frombuffer(b"ACDEFGHIKLMNPQRS", np.uint8), np.array([0, 8, 16]), device="cpu")
    operand = device.LevMasks(torch.zeros(1024, dtype=torch.uint8), 2, 8, np.zeros(256, np.uint8), 1)
    for name, call in (("residues", lambda: device.lev_masks(ds)), ("residues", lambda: device.lev_masks(ds, np.zeros(256, np.uint8))),
                       ("match masks", lambda: device.lev_rect(operand)),
                       ("match masks", lambda: device.lev_rect(operand, 0, 1, 1, 2, kind=_capi.DA_OUT_COMPACT))):
        with pytest.raises(_capi.DynaAlignError) as e:
            call()
        assert (e.value.code, str(e.value)) == (NO_DEVICE, text % name)


# ---- codes, values and the rank table ------------------------------------------------------------------------------------------------------

def test_every_possible_code_is_in_the_rank_tables_domain_with_its_value(lib, da):
    ranks, distinct = da.nw_code_ranks(127)
    pairs = [(num, ln) for ln in range(1, 128) for num in range(ln + 1)]            # (L - d, L): 1 <= L <= 127, 0 <= L - d <= L
    assert len(pairs) == 127 * 128 // 2 + 127 and (1, 1) in pairs                  # 0x0101, the code of two empty strings: the value 1.0
    # the table's domain (da_nw_code_ranks(127)): low byte 1 .. 254, numerator <= min(low byte, 127)
    assert all(1 <= ln <= 254 and 0 <= num <= min(ln, 127) and (num << 8 | ln) < 65536 for num, ln in pairs)
    by_value = {}
    for num, ln in pairs:
        by_value.setdefault(num / ln, set()).add(int(ranks[num << 8 | ln]))
    assert all(len(r) == 1 for r in by_value.values())                              # equal values, equal ranks: 10/20 and 5/10 are one key
    order = sorted(by_value)
    got = [next(iter(by_value[v])) for v in order]
    assert got == sorted(got) and len(set(got)) == len(got) and max(got) < distinct <= 65536     # a larger value, a larger rank
    assert ranks[10 << 8 | 20] == ranks[5 << 8 | 10] == ranks[1 << 8 | 2] and ranks[0x0101] == ranks[127 << 8 | 127] == max(got)
    assert ranks[0 << 8 | 1] == ranks[0 << 8 | 127] == min(got)
    # the value of a code is Python's divide of its two integers: the library's (double)numerator / (double)length, read here from the
    # host-side table of da_nw_value_ranks (the widening table itself is internal; the GPU tests compare every widened value bit for bit)
    values, vrank = da.nw_value_ranks(127)
    assert all(values[vrank[ln, num]] == num / ln for num, ln in pairs)
    # and the largest code of a call lies below the bins its threshold step counts: (max_len << 8 | max_len) + 1, max_len at least 1
    for max_len in (1, 20, 127):
        assert max(num << 8 | ln for num, ln in pairs if ln <= max_len) == (max_len << 8 | max_len)
