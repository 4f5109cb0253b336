"""GPU tests of how the row expansion (minhash_kernels.hip k_expand_stream) deals its work: the output rows are cut into eight contiguous zones,
the copies of every unique string are listed per (zone, id), every zone has its own item list in table-row order with a prefix array, and one
ticket counter per zone serves all chunk launches of a call through a bounded compare-and-swap.  The lists are read back through
da_debug_expand_lists and checked as sets; the whole n x n matrix of the `rows` and `rowspipe` forms must stay bit-identical to the direct route
where zones are empty, where one zone holds all the heavy copies (the other zones' workgroups must steal), over several chunk launches on the two
alternating streams, with the uint16 table, in a padded output, and in the rectangular (two-set) form."""
import ctypes
import os

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
ES_COPIES = 4


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    from dynaalign_amd import _capi
    assert _capi.load().da_device_count() > 0
    return dynaalign_amd


class env:
    def __init__(self, **kv):
        self.kv = {k: str(v) for k, v in kv.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def run(seqs, k, n_hash, seed=12345, out=None, **switches):
    import torch
    from dynaalign_amd import device
    import dynaalign_amd as da_
    res, off = O.pack(seqs)
    ds = device.DeviceSequences(np.asarray(res, np.uint8), np.asarray(off, np.int64))
    seeds = da_.hash_family_seeds(seed, n_hash)
    with env(**switches):
        got = device.similarity_mh(ds, k, n_hash, seeds, out=out)
        torch.cuda.synchronize()
        route = device.mh_last_route()
    return got.cpu().numpy(), route


def oracle_expanded(seqs, k, n_hash, seed=12345):
    """the oracle on the unique strings, indexed out to all n rows (a value depends on the two strings only)"""
    uniq = sorted(set(seqs))
    at = {u: i for i, u in enumerate(uniq)}
    uid = np.array([at[s] for s in seqs])
    rc, m = O.similarity_mh(uniq, k, n_hash, O.seeds(seed, n_hash))
    assert rc == 0
    return np.asarray(m)[np.ix_(uid, uid)]


def pool_of(rng, U, length=20):
    """exactly U distinct strings: random ones and one-letter mutants of them"""
    pool, seen = [], set()
    while len(pool) < U:
        if pool and rng.rand() < 0.5:
            s = bytearray(pool[rng.randint(len(pool))], "ascii")
            s[rng.randint(length)] = AA[rng.randint(20)]
            s = s.decode()
        else:
            s = "".join(map(chr, AA[rng.randint(0, 20, length)]))
        if s not in seen:
            seen.add(s)
            pool.append(s)
    return pool


def duplicated(rng, U, extra=None):
    pool = pool_of(rng, U)
    seqs = pool + [pool[q] for q in rng.randint(0, U, U if extra is None else extra)]   # every string at least once
    rng.shuffle(seqs)
    return seqs


# ---- the lists ----------------------------------------------------------------------------------------------------------------------------------

def zoned_lists(uidx, U, zones):
    """da_debug_expand_lists: the copy lists of `zones` zones for the id map uidx, copied back"""
    import torch
    from dynaalign_amd import _capi
    lib = _capi.load()
    fn = lib.da_debug_expand_lists
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_void_p]
    fn.restype = ctypes.c_int
    n = len(uidx)
    off = (ctypes.c_int64 * 6)()
    used = ctypes.c_int(0)
    assert fn(None, n, U, zones, None, 0, ctypes.addressof(off), ctypes.addressof(used), None) == 0
    nbytes = int(off[4])
    d_uidx = torch.from_numpy(np.ascontiguousarray(uidx, np.int32)).cuda()
    scratch = torch.full((nbytes + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    assert scratch.data_ptr() % 16 == 0
    assert fn(d_uidx.data_ptr(), n, U, zones, scratch.data_ptr(), nbytes, ctypes.addressof(off), ctypes.addressof(used), None) == 0
    torch.cuda.synchronize()
    raw = scratch.cpu().numpy()
    assert (raw[nbytes:] == 0xA5).all()                                # nothing written past the size the callers allocate
    K = used.value * U
    cstart = raw[off[0]:off[0] + 4 * (K + 1)].view(np.uint32).astype(np.int64)
    zstart = raw[off[1]:off[1] + 4 * (K + 1)].view(np.uint32).astype(np.int64)
    cpos = raw[off[2]:off[2] + 4 * n].view(np.int32).astype(np.int64)
    items = raw[off[3]:off[3] + 8 * int(zstart[K])].view(np.int32).reshape(-1, 2).astype(np.int64)
    return dict(zones=used.value, Z=int(off[5]), cstart=cstart, zstart=zstart, cpos=cpos, items=items)


def check_lists(uidx, U, L):
    n, zones, Z = len(uidx), L["zones"], L["Z"]
    cstart, zstart, cpos, items = L["cstart"], L["zstart"], L["cpos"], L["items"]
    assert Z == -(-n // zones)
    zone_of = np.arange(n) // Z
    # the counts per (zone, id) and both prefix arrays
    cnt = np.bincount(zone_of * U + uidx, minlength=zones * U)
    assert np.array_equal(cstart, np.concatenate([[0], np.cumsum(cnt)])) and cstart[-1] == n
    per_key = -(-cnt // ES_COPIES)
    assert np.array_equal(zstart, np.concatenate([[0], np.cumsum(per_key)])) and zstart[-1] == len(items)
    # cpos: a permutation of the rows, every key's range holding exactly its copies (all of its zone, all of its id)
    assert np.array_equal(np.sort(cpos), np.arange(n))
    key_of_slot = np.repeat(np.arange(zones * U), cnt)
    assert np.array_equal(zone_of[cpos] * U + uidx[cpos], key_of_slot)
    # the items: zone z owns items [zstart[z U], zstart[(z + 1) U]), ascending by table row, the items of row r at [zstart[z U + r], zstart[z U + r + 1])
    seen = np.zeros(n, np.int64)
    for z in range(zones):
        lo, hi = zstart[z * U], zstart[(z + 1) * U]
        ids = items[lo:hi, 0]
        assert (np.diff(ids) >= 0).all()
        assert np.array_equal(ids, np.repeat(np.arange(U), per_key[z * U:(z + 1) * U]))
        for k in range(lo, hi):
            r, first = items[k]
            key = z * U + r
            assert zstart[key] <= k < zstart[key + 1] and first == (k - zstart[key]) * ES_COPIES
            c0, c1 = cstart[key] + first, min(cstart[key] + first + ES_COPIES, cstart[key + 1])
            assert c0 < c1
            rows = cpos[c0:c1]
            assert (uidx[rows] == r).all() and (rows // Z == z).all()
            seen[rows] += 1
    assert (seen == 1).all()                                           # every (id, copy) in exactly one item


def uidx_cases():
    rng = np.random.RandomState(5)
    out = {}
    out["n5"] = (np.array([0, 1, 0, 2, 1]), 3)
    out["n37"] = (np.concatenate([[0, 1, 2], rng.randint(0, 3, 34)]), 3)
    u = np.arange(4099) % 4009                                         # U = 4010: ids 0 ... 4008 once, then id 4009 with 90 copies, all in the
    u[4099 - 90:] = 4009                                               # last eighth (zone 7: rows 3591 ...)
    out["n4099_heavy_last_zone"] = (u, 4010)
    out["n4096_every_id_in_every_zone"] = (np.concatenate([rng.permutation(512) for _ in range(8)]), 512)
    return out


@pytest.mark.parametrize("zones", [8, 1])
@pytest.mark.parametrize("case", sorted(uidx_cases()))
def test_zoned_lists(da, case, zones):
    uidx, U = uidx_cases()[case]
    uidx = np.asarray(uidx, np.int64)
    assert len(np.unique(uidx)) == U and uidx.max() == U - 1
    if case == "n4099_heavy_last_zone":
        assert (np.flatnonzero(uidx == U - 1) // 513 == 7).all() and (uidx == U - 1).sum() == 90
    if case == "n4096_every_id_in_every_zone":
        assert all(len(np.unique(uidx[z * 512:(z + 1) * 512])) == 512 for z in range(8))
    L = zoned_lists(uidx, U, zones)
    assert L["zones"] == zones
    check_lists(uidx, U, L)


def test_default_is_zoned_or_not_as_documented(da):
    """what a call uses (zones = 0): eight zones unless DYNAALIGN_MH_EXPAND_ZONES=1"""
    uidx, U = uidx_cases()["n37"]
    assert zoned_lists(uidx, U, 0)["zones"] == 8
    with env(DYNAALIGN_MH_EXPAND_ZONES=1):
        assert zoned_lists(uidx, U, 0)["zones"] == 1


# ---- the whole matrix ---------------------------------------------------------------------------------------------------------------------------

DEDUP = dict(DYNAALIGN_MH_DEDUP_MIN_N=1, DYNAALIGN_PLANE_BITS=12)
FORMS = {"rows": "rows", "rowspipe": "rows, pipelined"}


def case_seqs(case):
    rng = np.random.RandomState({"a": 1537, "b": 3100, "c": 1200, "d": 1151, "e": 1300}[case])
    if case == "a":
        return duplicated(rng, 1537), 500, {}
    if case == "b":
        return duplicated(rng, 3100), 500, dict(DYNAALIGN_MH_PIPE_HEAD=1, DYNAALIGN_MH_PIPE_STEP=1)
    if case == "c":
        # three strings with 70 copies each (69 extra rows), every copy inside zone 6: n = 1200 + 1000 = 2200 rows, Z = 275, zone 6 = rows
        # 1650 ... 1924; the other strings' rows fill the rest
        pool = pool_of(rng, 1200)
        heavy, rest = pool[:3], pool[3:]
        others = rest + [rest[q] for q in rng.randint(0, len(rest), 2200 - 210 - len(rest))]
        rng.shuffle(others)
        block = [h for h in heavy for _ in range(70)]
        rng.shuffle(block)
        seqs = others[:1655] + block + others[1655:]
        assert len(seqs) == 2200 and all(1650 <= i < 1925 for i, s in enumerate(seqs) if s in heavy)
        return seqs, 500, {}
    if case == "d":
        return duplicated(rng, 1151), 512, {}
    if case == "e":
        return duplicated(rng, 1300, extra=1301), 500, {}                # n = 2601: odd
    raise KeyError(case)


@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e"])
def test_row_forms_whole_matrix(da, case):
    import torch
    seqs, n_hash, more = case_seqs(case)
    n, U = len(seqs), len(set(seqs))
    assert U == {"a": 1537, "b": 3100, "c": 1200, "d": 1151, "e": 1300}[case]
    direct, droute = run(seqs, 4, n_hash, DYNAALIGN_MH_NO_DEDUP=1)
    assert not droute["dedup"]
    if case == "a":
        assert n == 2 * U and same(direct, oracle_expanded(seqs, 4, n_hash))
    for form, name in FORMS.items():
        out = buf = None
        if case == "e":                                                 # an odd n in an even, padded leading dimension
            assert n % 2 == 1
            buf = torch.full((n, n + 5), -1.0, dtype=torch.float64, device="cuda")
            out = buf[:, :n]
        got, route = run(seqs, 4, n_hash, out=out, DYNAALIGN_MH_EXPAND=form, **DEDUP, **more)
        assert route["dedup"] and route["unique"] == U and route["expansion"] == name, route
        if case == "b" and form == "rowspipe":
            assert route["chunks"] >= 4, route
        assert same(got, direct), (case, form)
        if buf is not None:
            assert bool((buf[:, n:] == -1.0).all())


def test_rectangular_form_against_the_square_block(da):
    """similarityMH_cross through the duplicate route (the rectangular row expansion: zones over the m rows of x, one launch) against rows
    [0, m) x columns [m, m + n) of the square call's direct route"""
    import torch
    from dynaalign_amd import device
    import dynaalign_amd as da_
    rng = np.random.RandomState(300)
    pool = pool_of(rng, 900)
    x = [pool[q] for q in rng.randint(0, 120, 300)]                     # m = 300 rows of 120 strings
    y = [pool[q] for q in rng.randint(60, 900, 2500)]                   # n = 2 500 of 840, sharing 60 with x
    assert len(set(x)) < 300 and len(set(y)) < 2500
    square, sroute = run(x + y, 4, 500, DYNAALIGN_MH_NO_DEDUP=1)
    assert not sroute["dedup"]
    seeds = da_.hash_family_seeds(12345, 500)
    sets = []
    for s in (x, y):
        res, off = O.pack(s)
        sets.append(device.DeviceSequences(np.asarray(res, np.uint8), np.asarray(off, np.int64)))
    with env(DYNAALIGN_MH_DEDUP_MIN_N=1, DYNAALIGN_MH_DEDUP_MAX_PCT=100):
        got = device.similarity_mh_cross(sets[0], sets[1], 4, 500, seeds)
        torch.cuda.synchronize()
        route = device.mh_cross_last_route()
    assert route["dedup"] and (route["unique_x"], route["unique_y"]) == (len(set(x)), len(set(y))), route
    assert same(got.cpu().numpy(), square[:300, 300:])
