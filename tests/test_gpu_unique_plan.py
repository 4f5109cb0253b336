"""GPU tests of the duplicate plan on its own (nw_kernels.hip k_dd_*, da_dev_unique_plan) and of the sorted order the ordered DP's prefix sharing
uses (launch_nw_sort_unique through da_debug_nw_sort_unique).  No n x n matrix is computed: every field the plan hands out -- d_uidx, d_ufirst,
d_ulast, d_uoffsets, d_ubytes, d_minfirst, d_maxlast -- is compared as integers with the Python model (tests/unique_plan_model.py) at the sizes
where the plan changes its path (the one-workgroup scans' steps of 1024, the three-launch scans from 8192 elements on, over n and over U), on
degenerate inputs, on string contents that a careless compare or hash would confuse, and on probe chains built on purpose (a chain that wraps
from the table's last slot to slot 0, a chain of 200).  The workspace carries 4096 sentinel bytes behind da_dev_unique_plan_bytes."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
import unique_plan_model as P
from test_gpu_mh_dedup_order import FIRST, MULTI_FIRST, ZONED, check_ids, dedup_ids

pytestmark = pytest.mark.gpu

GUARD, FILL = 4096, 0xA5


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    from dynaalign_amd import _capi
    assert _capi.load().da_device_count() > 0
    return dynaalign_amd


def plan_bytes(seqs):
    from dynaalign_amd import _capi
    return int(_capi.load().da_dev_unique_plan_bytes(len(seqs), sum(map(len, seqs))))


def device_plan(seqs, work=None):
    """da_dev_unique_plan on seqs in a sentinel-filled workspace (or in `work`, as another plan left it) -> the plan's fields on the host"""
    import torch
    from dynaalign_amd import _capi
    lib = _capi.load()
    res, off = O.pack(seqs)
    n, total = len(seqs), int(off[-1])
    d_res = torch.from_numpy(np.asarray(res, np.uint8).copy()).cuda()
    d_off = torch.from_numpy(np.asarray(off, np.int64).copy()).cuda()
    need = int(lib.da_dev_unique_plan_bytes(n, total))
    if work is None:
        work = torch.full((need + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert work.numel() >= need + GUARD and work.data_ptr() % 256 == 0
    work[need:] = FILL                                                             # the guard starts where THIS plan's workspace ends
    c = _capi.DaUniquePlan()
    c.struct_size = ctypes.sizeof(_capi.DaUniquePlan)
    _capi.check(lib.da_dev_unique_plan(d_res.data_ptr(), d_off.data_ptr(), n, total, work.data_ptr(), need, ctypes.addressof(c), None))
    torch.cuda.synchronize()
    host = work.cpu().numpy()
    assert (host[need:] == FILL).all(), "bytes behind da_dev_unique_plan_bytes were written"
    U = int(c.unique)
    assert int(c.n) == n and 1 <= U <= n

    def field(ptr, dtype, count):
        o, nb = int(ptr) - work.data_ptr(), count * np.dtype(dtype).itemsize
        assert 0 <= o and o + nb <= need and o % np.dtype(dtype).itemsize == 0
        return host[o:o + nb].view(dtype).astype(np.int64)

    nb = -(-U // 64)
    uoff = field(c.d_uoffsets, np.int64, U + 1)
    assert 0 <= uoff[-1] <= total
    return {"U": U, "uidx": field(c.d_uidx, np.int32, n), "ufirst": field(c.d_ufirst, np.int32, U), "ulast": field(c.d_ulast, np.int32, U),
            "uoffsets": uoff, "ubytes": field(c.d_ubytes, np.uint8, int(uoff[-1])).astype(np.uint8).tobytes(),
            "minfirst": field(c.d_minfirst, np.int32, nb), "maxlast": field(c.d_maxlast, np.int32, nb)}


def assert_plan(got, seqs):
    want = P.plan_model(seqs)
    assert got["U"] == want["U"]
    for f in ("uidx", "ufirst", "ulast", "uoffsets", "minfirst", "maxlast"):
        assert got[f].shape == want[f].shape, f
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, "%s differs at %d places, first at %d: got %d, want %d" % (f, bad.size, bad[0], got[f][bad[0]], want[f][bad[0]])
    assert got["ubytes"] == want["ubytes"]
    return want


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", sorted(P.size_cases()))
def test_plan_at_the_sizes_where_its_path_changes(da, case):
    seqs, n, U = P.size_cases()[case]
    want = assert_plan(device_plan(seqs), seqs)
    assert len(seqs) == n and want["U"] == U
    if n >= 63:
        assert 0 < want["M"] < U                                                   # multi- and single-copy strings: both flag arrays are scanned


@pytest.mark.parametrize("case", sorted(P.degenerate_cases()))
def test_plan_on_degenerate_inputs(da, case):
    seqs = P.degenerate_cases()[case]
    want = assert_plan(device_plan(seqs), seqs)
    U, M = want["U"], want["M"]
    assert {"all_equal_8192": (U, M) == (1, 1), "all_distinct_8192": (U, M) == (8192, 0), "every_string_twice": U == M == 4500,
            "five_empty": U == 1 and want["uoffsets"].tolist() == [0, 0]}[case]


@pytest.mark.parametrize("case", sorted(P.content_cases()))
def test_plan_on_string_contents(da, case):
    seqs = P.content_cases()[case]
    assert_plan(device_plan(seqs), seqs)


def test_probe_chains(da):
    """a chain that must wrap from the last slot to slot 0, strings displaced from slots 0 and 1 by it, a chain of 200 entries"""
    seqs, groups = P.probe_chain_case()
    n = len(seqs)
    ts = P.table_size(n)
    assert (n, ts) == (600, 2048)
    wrap, slots = groups["wrap"]
    assert len(set(wrap)) == 48 > len(slots) == 3 and all(P.dd_hash(s) & (ts - 1) in (ts - 3, ts - 2, ts - 1) for s in wrap)
    assert sorted({seqs.count(s) for s in wrap}) == [1, 2, 3]
    displaced, _ = groups["displaced"]
    assert len(set(displaced)) == 24 and all(P.dd_hash(s) & (ts - 1) in (0, 1) for s in displaced)
    chain, _ = groups["chain"]
    assert len(set(chain)) == 200 and len({P.dd_hash(s) & (ts - 1) for s in chain}) == 1
    assert len(set(seqs)) == 48 + 24 + 200 + 300
    assert_plan(device_plan(seqs), seqs)


# ---- a workspace that another plan has used --------------------------------------------------------------------------------------------------------

def test_second_plan_in_a_used_workspace(da):
    """the hash table's words are recycled as the wide scans' block sums, and every array is sized for the call's own n: a smaller plan built where
    a larger one stood must not read what that one left"""
    import torch
    big = P.size_cases()["n20000_u12353"][0]
    later = [P.size_cases()[k][0] for k in ("n9217", "n20000_u8192", "n8191", "n1025", "n65")] + [P.probe_chain_case()[0], P.degenerate_cases()["five_empty"]]
    need = max(plan_bytes(s) for s in [big] + later)
    work = torch.full((need + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    for seqs in later:
        assert_plan(device_plan(big, work), big)
        assert_plan(device_plan(seqs, work), seqs)
    fresh = device_plan(later[0])
    again = device_plan(later[0], work)
    assert all(np.array_equal(fresh[f], again[f]) for f in ("uidx", "ufirst", "ulast", "uoffsets", "minfirst", "maxlast")) and fresh["ubytes"] == again["ubytes"]


# ---- the other id orders at the same sizes -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", sorted(P.order_cases()))
def test_id_orders_across_the_scan_switch(da, case):
    seqs = P.order_cases()[case]
    plan = device_plan(seqs)
    for order, zones in ((MULTI_FIRST, 1), (FIRST, 1), (ZONED, 8), (ZONED, 1)):
        uidx, U, M = dedup_ids(seqs, order, zones)
        check_ids(seqs, uidx, U, M, order, zones)
        if order == MULTI_FIRST:
            assert U == plan["U"] and np.array_equal(uidx, plan["uidx"])


# ---- the sorted order of the unique strings (prefix sharing) -----------------------------------------------------------------------------------------

def sort_unique(strings):
    """da_debug_nw_sort_unique on strings of residue codes -> (perm[n], lcp[n])"""
    import torch
    from dynaalign_amd import _capi
    fn = _capi.load().da_debug_nw_sort_unique
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    res, off = O.pack(strings)
    n = len(strings)
    d_res = torch.from_numpy(np.asarray(res, np.uint8).copy()).cuda()
    d_off = torch.from_numpy(np.asarray(off, np.int64).copy()).cuda()
    d_perm = torch.full((n + 4,), -9, dtype=torch.int32, device="cuda")
    d_lcp = torch.full((n + 4,), 0xEE, dtype=torch.uint8, device="cuda")
    assert fn(d_res.data_ptr(), d_off.data_ptr(), n, d_perm.data_ptr(), d_lcp.data_ptr(), None) == 0
    torch.cuda.synchronize()
    perm, lcp = d_perm.cpu().numpy().astype(np.int64), d_lcp.cpu().numpy().astype(np.int64)
    assert (perm[n:] == -9).all() and (lcp[n:] == 0xEE).all()
    return perm[:n], lcp[:n]


def sort_input(n):
    """n strings of codes 0 ... 23 and 0 ... 24 residues: families that share their first 12 residues (one key of the two-key sort) and differ only
    behind them, lengths 12, 13 and 24 exactly, prefixes of other strings, the empty string, duplicates; in random order"""
    rng = np.random.RandomState(5500 + n)
    if n == 1:
        return [bytes(rng.randint(0, 24, 24).astype(np.uint8))]
    if n == 2:
        head = bytes(rng.randint(0, 24, 12).astype(np.uint8))
        return [head + b"\x00", head]                                              # an extension in front of its 12-residue prefix
    out = [b"", b"", b"\x00", b"\x00\x00", b"\x17", b"\x17" * 24, b"\x00" * 24, b"\x00" * 12, b"\x00" * 13]
    while len(out) < n:
        head = bytes(rng.randint(0, 24, 12).astype(np.uint8))
        out += [head, head + bytes([rng.randint(24)]), head[:rng.randint(0, 12)]]  # lengths 12 and 13, a proper prefix
        for _ in range(rng.randint(1, 6)):                                         # same first key, different second key
            out.append(head + bytes(rng.randint(0, 24, rng.randint(1, 13)).astype(np.uint8)))
        tail = bytes(rng.randint(0, 24, 12).astype(np.uint8))
        out += [head + tail, head + tail[:11] + bytes([(tail[11] + 1) % 24]), head + tail]   # 24 residues: the last one differs; a duplicate
        out.append(bytes(rng.randint(0, 24, rng.randint(0, 25)).astype(np.uint8)))
        out.append(out[rng.randint(len(out))])                                     # a duplicate of anything
    out = out[:n]
    return [out[q] for q in rng.permutation(n)]


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 5000])
def test_sorted_order_and_common_prefixes(da, n):
    strings = sort_input(n)
    assert len(strings) == n and max(map(len, strings)) <= 24 and all(max(s, default=0) <= 23 for s in strings)
    if n >= 255:
        assert {0, 12, 13, 24} <= {len(s) for s in strings} and len(set(strings)) < n
        assert len({s[:12] for s in strings if len(s) > 12}) < len({s for s in strings if len(s) > 12}) // 2
    perm, lcp = sort_unique(strings)
    assert np.array_equal(np.sort(perm), np.arange(n))
    ordered = [strings[q] for q in perm]
    # bytes compare like the two keys: position by position on the code, a string before its extensions
    bad = [pos for pos in range(1, n) if ordered[pos - 1] > ordered[pos]]
    assert not bad, "not sorted at position %d" % bad[0]
    assert lcp[0] == 0
    for pos in range(1, n):
        a, b = ordered[pos - 1], ordered[pos]
        k = 0
        while k < min(len(a), len(b)) and a[k] == b[k]:
            k += 1
        assert lcp[pos] == k, (pos, a, b)
