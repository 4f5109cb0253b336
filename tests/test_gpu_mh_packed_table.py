"""GPU tests of the packed count table of the duplicate route's row forms (api.cpp mh_rows_pipe / mh_one_stream with `rows`): for n_hash <= 511,
12 code planes and no heavy / rare split, the compare kernels write the U x U table as low bytes + a bit plane for bit 8 (da_common.hpp pk_*)
and k_expand_stream copies its rows into LDS as they are.  The whole n x n matrix must be bit-identical to the direct route and to the oracle
at the table's tile and bit-plane edges (U around 1024, an odd U), with counts that need bit 8 (near-duplicates, the diagonal at n_hash = 511),
and where the table stays uint16 (n_hash = 512, the split)."""
import os

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)


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


def run(seqs, k, n_hash, seed=12345, **switches):
    import torch
    from dynaalign_amd import device
    import dynaalign_amd as da_
    res, off = O.pack(seqs)
    ds = device.DeviceSequences(np.asarray(res, np.uint8), np.asarray(off, np.int64))
    seeds = da_.hash_family_seeds(seed, n_hash)
    with env(**switches):
        got = device.similarity_mh(ds, k, n_hash, seeds)
        torch.cuda.synchronize()
        route = device.mh_last_route()
    return got.cpu().numpy(), dict(route, packed_table=table_packed())


def table_packed():
    """da_debug_mh_last_table_packed: did this thread's last similarityMH call keep its count table at 9 bits per count?"""
    import ctypes
    from dynaalign_amd import _capi
    lib = _capi.load()
    lib.da_debug_mh_last_table_packed.argtypes = [ctypes.POINTER(ctypes.c_int)]
    lib.da_debug_mh_last_table_packed.restype = ctypes.c_int
    v = ctypes.c_int(-1)
    assert lib.da_debug_mh_last_table_packed(ctypes.byref(v)) == 0
    return bool(v.value)


def oracle_expanded(seqs, k, n_hash, seed=12345):
    """the oracle on the unique strings, indexed out to all n rows (a value depends on the two strings only)"""
    uniq = sorted(set(seqs))
    at = {u: i for i, u in enumerate(uniq)}
    uid = np.array([at[s] for s in seqs])
    rc, m = O.similarity_mh(uniq, k, n_hash, O.seeds(seed, n_hash))
    assert rc == 0
    return np.asarray(m)[np.ix_(uid, uid)]


def pool_of(rng, U, length=20):
    """exactly U distinct strings: random ones and one-letter mutants of them (similarities above 0.5: counts with bit 8 set at
    n_hash ~ 500)"""
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


def duplicated(rng, U):
    pool = pool_of(rng, U)
    seqs = pool + [pool[q] for q in rng.randint(0, U, U)]            # n = 2 U: every string at least once, half of them twice or more
    rng.shuffle(seqs)
    return seqs


DEDUP = dict(DYNAALIGN_MH_DEDUP_MIN_N=1, DYNAALIGN_PLANE_BITS=12)   # 12 code planes even where fewer would do (the packed table needs them)
FORMS = {"rows": "rows", "rowspipe": "rows, pipelined"}


@pytest.mark.parametrize("n_hash,U", [(500, 1023), (500, 1024), (500, 1025), (500, 1151), (500, 1537),
                                      (511, 1025), (511, 1151), (512, 1025), (512, 1151)])
def test_row_forms_whole_matrix(da, n_hash, U):
    rng = np.random.RandomState(U + n_hash)
    seqs = duplicated(rng, U)
    direct, droute = run(seqs, 4, n_hash, DYNAALIGN_MH_NO_DEDUP=1)
    assert not droute["dedup"]
    want = oracle_expanded(seqs, 4, n_hash)
    assert same(direct, want)
    assert (want[~np.eye(len(seqs), dtype=bool)] * n_hash > 255.5).any()   # off-diagonal counts that need bit 8
    for form, name in FORMS.items():
        got, route = run(seqs, 4, n_hash, DYNAALIGN_MH_EXPAND=form, **DEDUP)
        assert route["dedup"] and route["unique"] == U and route["expansion"] == name, route
        assert route["plane_bits"] == 12 and not route["split"], route
        assert route["packed_table"] == (n_hash <= 511), route             # 512: counts need 10 bits, the table stays uint16
        assert same(got, direct), (form, n_hash, U)
    assert not droute["packed_table"]


def test_band_kernel_walks_several_tiles_per_workgroup(da):
    """the band kernel stages a tile in the ring slot of its last stage while the next tile's first stages land in the other two: with U = 6000
    and one workgroup per CU (DYNAALIGN_MH_PIPE_WG=1) the chunk after the first holds ~780 tile ids, ~3 per workgroup"""
    rng = np.random.RandomState(6000)
    seqs = duplicated(rng, 6000)
    direct, _ = run(seqs, 4, 500, DYNAALIGN_MH_NO_DEDUP=1)
    got, route = run(seqs, 4, 500, DYNAALIGN_MH_EXPAND="rowspipe", DYNAALIGN_MH_PIPE_WG=1, **DEDUP)
    assert route["expansion"] == "rows, pipelined" and route["chunks"] >= 2 and route["packed_table"], route
    assert same(got, direct)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_split_keeps_the_uint16_table(da, form):
    """the heavy / rare split adds list incidences into table entries: its table stays uint16 in both row forms"""
    rng = np.random.RandomState(23)
    par = AA[rng.randint(0, 20, (6, 400))]
    pool = set()
    while len(pool) < 3500:
        p, at = rng.randint(6), rng.randint(0, 380)
        w = par[p, at:at + 20].copy()
        hit = rng.rand(20) < 0.03
        w[hit] = AA[rng.randint(0, 20, hit.sum())]
        pool.add(w.tobytes().decode())
    pool = sorted(pool)
    seqs = [pool[q] for q in rng.randint(0, len(pool), 7000)]
    direct, _ = run(seqs, 4, 500, DYNAALIGN_MH_NO_DEDUP=1, DYNAALIGN_MH_NO_SPARSE=1, DYNAALIGN_MH_NO_HYBRID=1)
    got, route = run(seqs, 4, 500, DYNAALIGN_MH_HYBRID_MIN_N=256, DYNAALIGN_MH_HYBRID_DEDUP=1, DYNAALIGN_MH_DEDUP_MIN_N=1,
                     DYNAALIGN_MH_DEDUP_MAX_PCT=100, DYNAALIGN_MH_EXPAND=form)
    assert route["dedup"] and route["split"] and route["expansion"] == FORMS[form] and not route["packed_table"], route
    assert same(got, direct)
