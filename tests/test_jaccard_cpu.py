"""CPU tests of the exact Jaccard index of k-shingle sets: jaccard_dense (the package's statement of the definition) against hand-written cases
and against Python sets of byte slices written here, the new symbols, every validation path of the C ABI -- status, text and order, all
before a device is needed -- and the code / rank-table contract (every code the limits allow lies in the domain of da_nw_code_ranks(127) and
its value is the divide of its two integers).  No compute calls here."""
import inspect

import numpy as np
import pytest

import oracle_lib as O

SYMBOLS = ["da_similarity_jaccard", "da_similarity_jaccard_cross", "da_similarity_jaccard_cross_topk", "da_similarity_jaccard_knn",
           "da_similarity_jaccard_edges", "da_similarity_jaccard_edges_begin", "da_dev_jaccard_sets_ld", "da_dev_jaccard_sets", "da_dev_jaccard_rect"]
OK, EMPTY, BAD_K, NO_DEVICE, UNSUPPORTED, BAD_ARG = 0, 1, 2, 8, 10, 11
K_LIMIT = "the exact Jaccard index packs a shingle into one 64-bit key: k <= 8 (got 9)"
SECOND = "a nearest neighbour needs a second sequence"
TWO = "the threshold is a quantile of the strict upper triangle: need >= 2 sequences"


def too_long(i):
    return "sequence %d has 128 shingle positions: the exact Jaccard index takes at most 127 (length - k + 1 <= 127)" % i


@pytest.fixture(scope="module")
def lib(built):
    from dynaalign_amd import _capi
    return _capi.load()


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    return dynaalign_amd


# ---- the definition ------------------------------------------------------------------------------------------------------------------------

def test_jaccard_dense_hand_written_cases(da):
    J = da.jaccard_dense(["ABCDEF", "BCDEFG"], 3)
    assert J.dtype == np.float64 and J.shape == (2, 2)
    assert J[0, 1] == J[1, 0] == 3 / 5 and J[0, 0] == J[1, 1] == 1.0            # BCD CDE DEF of ABC .. EFG
    for k in range(1, 9):
        inter, union = da.jaccard_counts(["AAAAAAAA"], k)
        assert (inter[0, 0], union[0, 0]) == (1, 1)                                # one shingle at any k <= 8
    inter, union = da.jaccard_counts(["AAAAAAAA"], 9)
    assert (inter[0, 0], union[0, 0]) == (0, 0) and da.jaccard_dense(["AAAAAAAA"], 9)[0, 0] == 1.0
    J = da.jaccard_dense(["", "A", "AC", "ACDEFGHIK"], 4)
    assert np.array_equal(J, np.array([[1.0, 1, 1, 0], [1, 1, 1, 0], [1, 1, 1, 0], [0, 0, 0, 1]]))
    # bytes >= 0x80, str (latin-1) and bytes alike; FF FF FF FF is a shingle like any other
    a, b = b"AC\xff\xff\xff\xffDE", "AC\xff\xff\xff\xffDF"
    inter, union = da.jaccard_counts([a, b, b"\xff" * 6, "\x80\x81\x82\x83", b"\x80\x81\x82\x83\x84"], 4)
    assert (inter[0, 1], union[0, 1]) == (4, 6)                                     # AC\xff\xff C\xff\xff\xff \xff*4 \xff\xff\xffD  |  + 2 + 2 - 4
    assert (inter[0, 2], union[0, 2], inter[2, 2]) == (1, 5, 1)
    assert (inter[3, 4], union[3, 4]) == (1, 2)
    # the two-set form is the block of the square one
    x, y = ["ABCDEF", "", "QRS"], ["BCDEFG", "A", "ABCDEF", "QRSQRS"]
    assert np.array_equal(da.jaccard_dense(x, 3, y), da.jaccard_dense(x + y, 3)[:3, 3:])
    with pytest.raises(ValueError):
        da.jaccard_dense(["AC"], 0)


def test_jaccard_dense_against_python_sets(da):
    rng = np.random.RandomState(8)
    alphabet = [bytes([c]) for c in b"ACDEFG"] + [b"\xff", b"\x00", b"\x80"]
    seqs = [b"".join(alphabet[t] for t in rng.randint(0, len(alphabet), rng.randint(0, 24))) for _ in range(300)]
    for k in (1, 2, 3, 5, 8):
        sets = [{b[p:p + k] for p in range(len(b) - k + 1)} for b in seqs]
        inter, union = da.jaccard_counts(seqs, k)
        J = da.jaccard_dense(seqs, k)
        want_i = np.array([[len(a & b) for b in sets] for a in sets])
        want_u = np.array([[len(a | b) for b in sets] for a in sets])
        assert np.array_equal(inter, want_i) and np.array_equal(union, want_u)
        want = np.array([[(i / u) if u else 1.0 for i, u in zip(ri, ru)] for ri, ru in zip(want_i, want_u)])
        assert np.array_equal(J.view(np.uint64), want.view(np.uint64))
        assert np.array_equal(J, J.T) and np.all(np.diag(J) == 1.0)
        # the input has something of everything: shared shingles off the diagonal (at the small k), two empty sets, one empty set
        assert (union == 0).sum() > 0 and ((inter == 0) & (union > 0)).sum() > 0 and (k > 3 or (inter > 0).sum() > 2 * len(seqs))


# ---- symbols and mirror --------------------------------------------------------------------------------------------------------------------

def test_header_library_and_signatures_agree_on_the_jaccard_symbols(lib):
    from dynaalign_amd import _capi
    declared = _capi.header_symbols()
    for name in SYMBOLS:
        assert name in declared and name in _capi.SIGNATURES and hasattr(lib, name), name
    assert sorted(_capi.SIGNATURES) == declared
    assert lib.da_abi_version() == 2                                                  # entry points only: the version stays


def test_python_mirror_exports(da):
    from dynaalign_amd import device
    for name in ("jaccard_dense", "jaccard_counts", "similarityJaccard", "similarityJaccard_cross", "similarityJaccard_cross_topk",
                 "similarityJaccard_knn", "similarityJaccard_knn_edges", "similarityJaccard_edges"):
        assert name in da.__all__ and callable(getattr(da, name)), name
    params = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]      # noqa: E731
    none = inspect.Parameter.empty
    assert params(da.jaccard_dense) == [("sequences", none), ("k", none), ("y", None)]
    assert params(da.similarityJaccard) == [("sequences", none), ("k", 4)]
    assert params(da.similarityJaccard_cross) == [("x", none), ("y", none), ("k", 4)]
    assert params(da.similarityJaccard_cross_topk) == [("x", none), ("y", none), ("k", 4), ("top", 10)]
    assert params(da.similarityJaccard_knn) == [("sequences", none), ("k", 4), ("top", 10)]
    assert params(da.similarityJaccard_knn_edges) == [("sequences", none), ("k", 4), ("top", 10), ("mode", "union")]
    assert params(da.similarityJaccard_edges) == [("sequences", none), ("k", 4), ("thresh_p", 0.8)]
    assert [p for p, _ in params(device.jaccard_sets)] == ["ds", "k"]
    assert [p for p, _ in params(device.jaccard_rect)] == ["sets", "row_begin", "row_end", "col_begin", "col_end", "kind", "out"]


# ---- validation: status, text, order -- no device ------------------------------------------------------------------------------------------

def err(lib, rc):
    return rc, lib.da_last_error().decode("latin-1") if rc else ""


def p_(a):
    return None if a is None else a.ctypes.data


def square(lib, seqs, k, res=True, off=True, out=True):
    r, o = O.pack(seqs)
    buf = np.full(max(len(seqs), 1) ** 2, -7.0)
    return err(lib, lib.da_similarity_jaccard(p_(r if res else None), p_(o if off else None), len(seqs), k, p_(buf if out else None)))


def knn(lib, seqs, k, top, idx=True):
    r, o = O.pack(seqs)
    cnt = max(len(seqs), 1) * max(top, 1)
    ib, vb = np.full(cnt, -7, np.int32), np.full(cnt, -7.0)
    return err(lib, lib.da_similarity_jaccard_knn(r.ctypes.data, o.ctypes.data, len(seqs), k, top, p_(ib if idx else None), vb.ctypes.data))


def edges(lib, seqs, k, p, begin=False):
    import ctypes
    r, o = O.pack(seqs)
    thr, cnt = np.zeros(1), np.zeros(1, np.int64)
    if begin:
        h = ctypes.c_void_p()
        rc = lib.da_similarity_jaccard_edges_begin(r.ctypes.data, o.ctypes.data, len(seqs), k, p, ctypes.addressof(h), thr.ctypes.data, cnt.ctypes.data)
        if rc == OK:
            lib.da_edges_free(h)
        else:
            assert h.value is None
        return err(lib, rc)
    return err(lib, lib.da_similarity_jaccard_edges(r.ctypes.data, o.ctypes.data, len(seqs), k, p, thr.ctypes.data, cnt.ctypes.data, 0, None, None, None))


def cross(lib, x, y, k, topk=None, out=True):
    xr, xo = O.pack(x)
    yr, yo = O.pack(y)
    if topk is None:
        buf = np.full(max(len(x), 1) * max(len(y), 1), -7.0)
        return err(lib, lib.da_similarity_jaccard_cross(xr.ctypes.data, xo.ctypes.data, len(x), yr.ctypes.data, yo.ctypes.data, len(y), k,
                                                        p_(buf if out else None), 0))
    cnt = max(len(x), 1) * max(topk, 1)
    ib, vb = np.full(cnt, -7, np.int32), np.full(cnt, -7.0)
    return err(lib, lib.da_similarity_jaccard_cross_topk(xr.ctypes.data, xo.ctypes.data, len(x), yr.ctypes.data, yo.ctypes.data, len(y), k, topk,
                                                         p_(ib if out else None), vb.ctypes.data))


def passes(result):
    """the validation let the call through: it ran (a device is present) or stopped at the device check, the last one"""
    return result[0] in (OK, NO_DEVICE)


def test_one_set_validation_order_and_texts(lib, da, kats):
    e = kats["mh_errors"]
    long135, long134 = "AC" * 67 + "A", "AC" * 67
    two = ["ACDEFGHIK", "ACDEFGHIR"]
    calls = {"square": lambda s, k: square(lib, s, k), "knn": lambda s, k: knn(lib, s, k, 1), "edges": lambda s, k: edges(lib, s, k, 0.8),
             "edges_begin": lambda s, k: edges(lib, s, k, 0.8, begin=True)}
    for name, call in calls.items():
        assert call([], 4) == (EMPTY, e["empty"]), name
        assert call([], 0) == (EMPTY, e["empty"]), name                            # n before k
        assert call(two, 0) == (BAD_K, e["k"]) and call(two, -1) == (BAD_K, e["k"]), name
        assert call([long135], 0) == (BAD_K, e["k"]), name                         # k before the limits
        assert call(two, 9) == (UNSUPPORTED, K_LIMIT), name
        assert call(two + [long135], 9) == (UNSUPPORTED, K_LIMIT), name            # k > 8 before the lengths
        assert call(two + [long135], 8) == (UNSUPPORTED, too_long(3)), name
        assert call([long135] + two, 8) == (UNSUPPORTED, too_long(1)), name
        assert passes(call(two + [long134], 8)), name                              # 127 shingles: the limit itself
        assert passes(call(["A" * 127, "", "A"], 1)), name                         # 127 positions at k = 1; empty and short sequences are legal
    # NULL pointers after n and k, before the offsets
    assert square(lib, two, 4, res=False)[0] == BAD_ARG and square(lib, two, 4, out=False)[0] == BAD_ARG
    assert square(lib, two, 0, res=False) == (BAD_K, e["k"])
    assert square(lib, two, 4, off=False) == (BAD_ARG, "offsets is NULL")
    assert knn(lib, two, 4, 1, idx=False)[0] == BAD_ARG
    # decreasing offsets, before the limits
    r, o = O.pack(two + [long135])
    o = o.copy()
    o[1], o[2] = o[2], o[1]
    buf = np.full(9, -7.0)
    assert err(lib, lib.da_similarity_jaccard(r.ctypes.data, o.ctypes.data, 3, 9, buf.ctypes.data)) == (BAD_ARG, "offsets must be non-decreasing (sequence 1)")
    # the Python mirror raises the same
    for fn in (da.similarityJaccard, da.similarityJaccard_knn, da.similarityJaccard_knn_edges, da.similarityJaccard_edges):
        for seqs, k, code, msg in [([], 4, EMPTY, e["empty"]), (two, 0, BAD_K, e["k"]), (two, 9, UNSUPPORTED, K_LIMIT), (two + [long135], 8, UNSUPPORTED, too_long(3))]:
            with pytest.raises(da.DynaAlignError) as ei:
                fn(seqs, k)
            assert (ei.value.code, str(ei.value)) == (code, msg), (fn.__name__, k)


def test_knn_and_edges_checks_follow_the_shared_ones(lib, da):
    three = ["ACDEFGHIK", "ACDEFGHIR", "ACDEFGHIW"]
    for top in (0, 1, 2000):
        assert knn(lib, ["ACDE"], 4, top) == (BAD_ARG, SECOND)                     # n = 1: no neighbour, whatever top
    for top in (0, -1, 3, 4):
        assert knn(lib, three, 4, top) == (BAD_ARG, "top must be in 1 .. n - 1 (got top = %d, n = 3)" % top)
    many = ["ACDE"] * 1030
    assert knn(lib, many, 4, 1025) == (UNSUPPORTED, "top-k per row keeps its candidates in a fixed LDS buffer: top <= 1024 (got 1025)")
    assert knn(lib, many, 4, 1030)[0] == BAD_ARG                                    # top > n - 1 before top > 1024
    assert knn(lib, three, 9, 0) == (UNSUPPORTED, K_LIMIT)                          # the shared checks first
    assert passes(knn(lib, three, 4, 2))
    with pytest.raises(da.DynaAlignError) as ei:
        da.similarityJaccard_knn(["ACDE"], 4)
    assert (ei.value.code, str(ei.value)) == (BAD_ARG, SECOND)
    for begin in (False, True):
        assert edges(lib, ["ACDE"], 4, 0.8, begin) == (BAD_ARG, TWO)               # edges with n = 1
        assert edges(lib, ["ACDE"], 4, 1.5, begin) == (BAD_ARG, TWO)               # ... before thresh_p
        for p in (-0.1, 1.0001, float("nan")):
            assert edges(lib, three, 4, p, begin) == (BAD_ARG, "thresh_p must be in [0, 1]")
        assert edges(lib, three, 9, 1.5, begin) == (UNSUPPORTED, K_LIMIT)
        assert passes(edges(lib, three, 4, 0.0, begin)) and passes(edges(lib, three, 4, 1.0, begin))
    r, o = O.pack(three)
    assert lib.da_similarity_jaccard_edges(r.ctypes.data, o.ctypes.data, 3, 4, 0.8, None, None, 0, None, None, None) == BAD_ARG
    assert lib.da_similarity_jaccard_edges_begin(r.ctypes.data, o.ctypes.data, 3, 4, 0.8, None, None, None) == BAD_ARG


def test_two_set_validation(lib, da, kats):
    e = kats["mh_errors"]
    x, y = ["ACDEFGHIK", "ACDEFGHIR"], ["ACDEFGHIW", "ACDEFGHIK", "AC"]
    long135 = "AC" * 67 + "A"
    for topk in (None, 1):
        assert cross(lib, x, y, 0, topk) == (BAD_K, e["k"]) and cross(lib, [], [], -1, topk) == (BAD_K, e["k"])
        assert cross(lib, [], y, 4, topk) == (OK, "")                               # no rows: nothing to write
        assert cross(lib, x, y, 4, topk, out=False)[0] == BAD_ARG
        assert cross(lib, x, y, 9, topk) == (UNSUPPORTED, K_LIMIT)
        assert cross(lib, x + [long135], y, 8, topk) == (UNSUPPORTED, too_long(3))
        assert cross(lib, x, [long135] + y, 8, topk) == (UNSUPPORTED, too_long(1))
        assert cross(lib, x + [long135], [long135] + y, 8, topk) == (UNSUPPORTED, too_long(3))      # x before y
        assert passes(cross(lib, x, y + ["AC" * 67], 8, topk))
    assert cross(lib, x, [], 4) == (OK, "")                                          # an m x 0 matrix
    assert cross(lib, x, [], 4, 1) == (BAD_ARG, "top must be in 1 .. n (got top = 1, n = 0)")
    for top in (0, -1, 4):                                                          # top = 0, top = n + 1
        assert cross(lib, x, y, 4, top) == (BAD_ARG, "top must be in 1 .. n (got top = %d, n = 3)" % top)
    many = ["ACDE"] * 1030
    assert cross(lib, x, many, 4, 1025) == (UNSUPPORTED, "top-k per row keeps its candidates in a fixed LDS buffer: top <= 1024 (got 1025)")
    assert cross(lib, x, many, 9, 0) == (UNSUPPORTED, K_LIMIT)                      # the limits before top
    assert da.similarityJaccard_cross([], y, 4).shape == (0, 3) and da.similarityJaccard_cross(x, [], 4).shape == (2, 0)
    idx, val = da.similarityJaccard_cross_topk([], y, 4, 2)
    assert idx.shape == (0, 2) and val.shape == (0, 2)


def test_device_layer_argument_checks(lib):
    e = lambda rc: err(lib, rc)                                                     # noqa: E731
    assert [lib.da_dev_jaccard_sets_ld(ml, k) for ml, k in [(0, 4), (3, 4), (4, 4), (12, 2), (20, 4), (21, 4), (134, 8), (130, 4), (5, 0)]] == \
        [4, 4, 4, 12, 20, 20, 128, 128, 0]
    fake = 4096                                                                     # never dereferenced: every call below is refused first
    sets = lambda n, ml, k, keys=fake, ld=128, cnt=fake, res=fake: e(lib.da_dev_jaccard_sets(res, fake, n, ml, k, keys, ld, cnt, None))      # noqa: E731
    assert sets(0, 20, 4)[0] == EMPTY and sets(3, 20, 0)[0] == BAD_K and sets(0, 20, 0)[0] == EMPTY
    assert sets(3, 20, 4, keys=None)[0] == BAD_ARG and sets(3, 20, 4, cnt=None)[0] == BAD_ARG and sets(3, 20, 4, res=None)[0] == BAD_ARG
    assert sets(3, 20, 9) == (UNSUPPORTED, K_LIMIT)
    assert sets(3, 135, 8)[0] == UNSUPPORTED and sets(3, -1, 4)[0] == BAD_ARG
    assert sets(3, 20, 4, ld=16)[0] == BAD_ARG and sets(3, 20, 4, ld=129)[0] == BAD_ARG      # ld_keys too small / beyond the 128 slots
    assert sets(3, 20, 4, keys=fake + 2)[0] == BAD_ARG and sets(3, 20, 5, keys=fake + 4)[0] == BAD_ARG      # keys aligned to their size
    rect = lambda n=10, ld_keys=20, k=4, r=(0, 10), c=(0, 10), kind=1, out=fake, ld=10, keys=fake: e(      # noqa: E731
        lib.da_dev_jaccard_rect(keys, fake, n, ld_keys, k, r[0], r[1], c[0], c[1], kind, out, ld, None))
    assert rect(k=0)[0] == BAD_K and rect(k=9) == (UNSUPPORTED, K_LIMIT)
    assert rect(keys=None)[0] == BAD_ARG and rect(out=None)[0] == BAD_ARG and rect(n=-1)[0] == BAD_ARG
    assert rect(r=(-1, 3))[0] == BAD_ARG and rect(r=(4, 3))[0] == BAD_ARG and rect(r=(0, 11))[0] == BAD_ARG
    assert rect(c=(-1, 3))[0] == BAD_ARG and rect(c=(4, 3))[0] == BAD_ARG and rect(c=(0, 11))[0] == BAD_ARG
    assert rect(ld=9)[0] == BAD_ARG and rect(kind=2)[0] == BAD_ARG and rect(ld_keys=0)[0] == BAD_ARG and rect(ld_keys=129)[0] == BAD_ARG
    assert rect(out=fake + 1)[0] == BAD_ARG and rect(kind=0, out=fake + 4)[0] == BAD_ARG      # naturally aligned output
    assert rect(r=(3, 3)) == (OK, "") and rect(c=(10, 10), ld=0) == (OK, "")       # an empty rectangle is DA_OK, before any launch


# ---- codes, values and the rank table ------------------------------------------------------------------------------------------------------

def test_every_possible_code_is_in_the_rank_tables_domain_with_its_value(lib, da):
    ranks, distinct = da.nw_code_ranks(127)
    # (intersection, union) under the limits: two sets of ca, cb <= 127 shingles share i <= min(ca, cb), union = ca + cb - i
    pairs = {(i, ca + cb - i) for ca in range(128) for cb in range(ca, 128) for i in range(ca + 1)} - {(0, 0)}
    assert max(u for _, u in pairs) == 254 and max(i for i, _ in pairs) == 127 and len(pairs) == 254 + 127 * 127      # i = 0: u in 1 .. 254; i >= 1: u in i .. 254 - i
    # the table's domain: length 1 .. 254, matches <= min(length, 127)
    assert all(1 <= u <= 254 and 0 <= i <= min(u, 127) for i, u in pairs)
    assert (1, 1) in pairs                                                           # 0x0101, the code of two empty sets: the value 1.0
    by_value = {}
    for i, u in pairs:
        by_value.setdefault(i / u, set()).add(int(ranks[i << 8 | u]))
    assert all(len(r) == 1 for r in by_value.values())                              # equal values, equal ranks: 2/4 and 3/6 are one key
    order = sorted(by_value)
    got = [next(iter(by_value[v])) for v in order]
    assert got == sorted(got) and len(set(got)) == len(got) and max(got) < distinct <= 65536     # a larger value, a larger rank
    assert ranks[2 << 8 | 4] == ranks[3 << 8 | 6] == ranks[1 << 8 | 2] and ranks[0x0101] == ranks[127 << 8 | 127] == max(got)
    # the value of a code is Python's divide of its two integers: the library's (double)matches / (double)length, read here from the host-side
    # table of da_nw_value_ranks (the widening table itself is internal; the GPU tests compare every widened value bit for bit)
    values, vrank = da.nw_value_ranks(127)
    assert all(values[vrank[u, i]] == i / u for i, u in pairs)
    seqs = ["ABCDEF", "BCDEFG", "ABCDXY", "", "AB", "ABCDEFGHIJKLMNOP"]
    inter, union = da.jaccard_counts(seqs, 3)
    J = da.jaccard_dense(seqs, 3)
    for a in range(len(seqs)):
        for b in range(len(seqs)):
            assert J[a, b] == (inter[a, b] / union[a, b] if union[a, b] else 1.0)
