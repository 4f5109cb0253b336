"""GPU tests of the ORDERED unique table of similarityNW (da_dev_nw_unique_rows, k_nw_short's ordered mode) on occurrence patterns chosen on
purpose.  calculate_similarity is not symmetric, and cell (p, q) of the table -- calc(U_p, U_q) -- is needed when some copy of string p stands before
some copy of string q: ufirst[p] < ulast[q], or p == q.  The sweep skips whole tiles (minfirst[ti] >= maxlast[tj]) and whole rows of a tile
(ufirst[p] >= maxlast[tj]); on random shuffles neither skip fires between multi-copy strings, so here the rows are arranged so that they do, with
the unique count around the tile edges.  Every needed cell must hold the oracle's matches << 8 | length; every other cell holds that code or was
never written; nothing outside the table is written.  The same inputs then go through similarityNW's duplicate route, against the direct kernel."""
import numpy as np
import pytest

import oracle_lib as O
import unique_plan_model as P
from test_gpu_nw_dedup import ASYM_A, ASYM_B, both_routes, same

pytestmark = pytest.mark.gpu

SYMBOLS = "ARNDCQEGHILKMFPSTWYVBZX*"
SENTINEL = 0xFFFF                                                                 # matches = 255, length = 255: no alignment of <= 24 residues
UNIQUES = (64, 65, 127, 128, 129, 200)
ARRANGEMENTS = ("nested", "blocks", "straggler", "single_in_row_0", "reverse_straggler", "singles_behind_head")
MATRICES = (("BLOSUM62", 10, 4), ("BLOSUM45", 3, 1))


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    from dynaalign_amd import _capi
    assert _capi.load().da_device_count() > 0
    return dynaalign_amd


def peptides(U, max_len):
    """U distinct peptides of 1 ... max_len residues over all 24 symbols; the two asymmetric sequences, one residue and max_len residues first"""
    rng = np.random.RandomState(6600 + max_len)
    pool = [ASYM_A, ASYM_B, "W", (SYMBOLS[::-1])[:max_len]]
    seen = set(pool)
    sym = np.frombuffer(SYMBOLS.encode(), np.uint8)
    while len(pool) < U:
        if rng.rand() < 0.4:                                                       # a relative of an earlier one: a prefix with another tail
            base = pool[rng.randint(len(pool))]
            cut = rng.randint(0, len(base) + 1)
            s = (base[:cut] + bytes(sym[rng.randint(0, 24, rng.randint(0, max_len + 1))]).decode())[:max_len]
        else:
            s = bytes(sym[rng.randint(0, 24, rng.randint(1, max_len + 1))]).decode()
        if s and s not in seen:
            seen.add(s)
            pool.append(s)
    return pool


def arrange(name, uniq):
    """the rows of the input as indices into uniq"""
    U = len(uniq)
    twice = [k for k in range(U) for _ in range(2)]
    if name == "nested":                       # string k in rows k and n - 1 - k: every ordered pair of strings is needed
        return list(range(U)) + list(range(U))[::-1]
    if name == "blocks":                       # all copies of k before all copies of k + 1: only p <= q is needed, the lower triangle of tiles is skippable
        return twice
    if name == "straggler":                    # blocks, and the string of the last block has one more copy in row 0 (ids go by first occurrence: it
        return [U - 1] + twice                 # becomes id 0, whose COLUMN is then needed by every row, in a tile column otherwise skippable)
    if name == "single_in_row_0":              # blocks behind ONE single-copy string: numbered last, first occurrence 0 -- a row of the last tile
        return [U - 1] + twice[:-2]            # row that every column tile needs, while its own column is needed by no other row
    if name == "reverse_straggler":            # blocks, and a string of the first tile has one more copy in the last row: a column every row needs
        return twice + [3]
    if name == "singles_behind_head":          # multi-copy strings shuffled in a head, then single-copy strings only
        rng = np.random.RandomState(U)
        M = U // 2
        head = [k for k in range(M) for _ in range(3)]
        return [head[q] for q in rng.permutation(len(head))] + list(range(M, U))
    raise KeyError(name)


def oracle_codes(order, matrix, go, ge):
    """W[p][q] = matches << 8 | length of calc(order[p], order[q]), both triangles"""
    U = len(order)
    rc, mt, ln, _, msg = O.nw_rows(order, 0, U, matrix, go, ge)
    assert rc == 0, msg
    up = (mt.astype(np.int64) << 8) | ln.astype(np.int64)                          # [p][q] = calc(order[min], order[max])
    rc, mt, ln, _, msg = O.nw_rows(order[::-1], 0, U, matrix, go, ge)
    assert rc == 0, msg
    lo = ((mt.astype(np.int64) << 8) | ln.astype(np.int64))[::-1, ::-1]            # reversed list: [p][q] = calc(order[max], order[min])
    p, q = np.indices((U, U))
    return np.where(p <= q, up, lo)


def unique_rows(plan, U, matrix, go, ge, rank, world):
    """da_dev_nw_unique_rows into a sentinel-filled buffer with a padded leading dimension and two guard rows -> uint16 [rows + 2][ld]"""
    import torch
    from dynaalign_amd import device
    T = -(-U // 128)
    rows = U if world == 1 else -(-T // world) * 128
    ld = -(-U // 8) * 8 + 8
    buf = torch.full((rows + 2, ld), -1, dtype=torch.int16, device="cuda")
    device.nw_unique_rows(plan, 24, matrix, go, ge, rank, world, buf)
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(np.uint16).astype(np.int64), rows


@pytest.mark.parametrize("U", UNIQUES)
@pytest.mark.parametrize("arrangement", ARRANGEMENTS)
def test_ordered_table(da, arrangement, U):
    import torch
    from dynaalign_amd import device
    uniq = peptides(U, 24)
    assert len(set(uniq)) == U and {len(s) for s in uniq} >= {1, 24} and set("".join(uniq)) == set(SYMBOLS) and min(map(len, uniq)) == 1
    seqs = [uniq[k] for k in arrange(arrangement, uniq)]
    n = len(seqs)
    model = P.plan_model([s.encode() for s in seqs])
    assert model["U"] == U
    uf, ul = model["ufirst"], model["ulast"]
    order = [seqs[i] for i in uf]                                                  # the unique strings in id order
    need = (uf[:, None] < ul[None, :]) | np.eye(U, dtype=bool)
    tile = np.arange(U) // 64
    tile_skip = model["minfirst"][tile][:, None] >= model["maxlast"][tile][None, :]
    if arrangement == "nested":
        assert need.all()
    if arrangement == "blocks":
        assert np.array_equal(need, np.triu(np.ones((U, U), bool)))
        assert tile_skip[tile[:, None] > tile[None, :]].all()                      # every tile below the diagonal tiles
    if arrangement == "straggler":
        assert order[0] == uniq[U - 1] and need[:, 0].all() and not tile_skip[:, 0].any() and not need[U - 1, 1:U - 1].any()
    if arrangement == "single_in_row_0":
        assert order[U - 1] == uniq[U - 1] and need[U - 1].all() and need[:U - 1, U - 1].sum() == 0
    if arrangement == "reverse_straggler":
        assert need[:, 3].all() and not need[U - 1, 4:U - 1].any()
    if arrangement == "singles_behind_head":
        M = model["M"]
        assert M == U // 2 and not need[M:, :M].any() and np.array_equal(need[M:, M:], np.triu(np.ones((U - M, U - M), bool)))

    res, off = O.pack(seqs)
    ds = device.DeviceSequences(res, off)
    assert int(device.nw_encode(ds).item()) == 0
    plan = device.UniquePlan(ds.codes, ds.offsets, n, ds.total)
    torch.cuda.synchronize()
    assert plan.unique == U
    for matrix, go, ge in MATRICES:
        want = oracle_codes(order, matrix, go, ge)
        a, b = order.index(ASYM_A), order.index(ASYM_B)
        if (matrix, go, ge) == ("BLOSUM62", 10, 4):
            assert want[a, b] == (3 << 8 | 21) and want[b, a] == (4 << 8 | 21)
        for world in (1, 2, 3):
            seen = np.zeros((U, U), bool)
            for rank in range(world):
                got, rows = unique_rows(plan, U, matrix, go, ge, rank, world)
                assert (got[rows:] == SENTINEL).all() and (got[:, U:] == SENTINEL).all(), "written outside the table"
                local = np.arange(rows)
                glob = local if world == 1 else ((local // 128) * world + rank) * 128 + local % 128
                assert (got[:rows][glob >= U] == SENTINEL).all(), "rows past the table were written"
                inside = glob < U
                g, w = got[:rows][inside][:, :U], want[glob[inside]]
                nd = need[glob[inside]]
                bad = np.argwhere(nd & (g != w))
                assert bad.size == 0, "needed cell (%d, %d): got %#x, want %#x (%s, world %d rank %d)" % (
                    glob[inside][bad[0][0]], bad[0][1], g[tuple(bad[0])], w[tuple(bad[0])], matrix, world, rank)
                assert ((g == w) | (g == SENTINEL))[~nd].all(), "a cell no pair needs holds neither its code nor the sentinel"
                assert not seen[glob[inside]].any()
                seen[glob[inside]] = True
            assert seen.all()                                                      # the ranks' units cover every row once


@pytest.mark.parametrize("U", UNIQUES)
@pytest.mark.parametrize("arrangement", ARRANGEMENTS)
def test_whole_route_on_the_same_arrangements(da, monkeypatch, arrangement, U):
    """similarityNW through the duplicate route (sequences <= 20 residues: the prefix-sharing kernel, then without the sharing) against the direct
    kernel, bit for bit"""
    from dynaalign_amd import device
    uniq = peptides(U, 20)
    seqs = [uniq[k] for k in arrange(arrangement, uniq)]
    assert max(map(len, seqs)) == 20 and len(seqs) <= 600 and 100 * U <= 85 * len(seqs)
    monkeypatch.setenv("DYNAALIGN_NW_DEDUP_MIN_N", "1")
    for args in MATRICES:
        got, direct = both_routes(da, seqs, *args)
        assert same(got, direct), (arrangement, U, args)
        monkeypatch.setenv("DYNAALIGN_NW_NO_PREFIX_SHARE", "1")
        plain = np.asarray(da.similarityNW(seqs, *args))
        route = device.nw_last_route()
        monkeypatch.delenv("DYNAALIGN_NW_NO_PREFIX_SHARE")
        assert route["dedup"] and route["unique"] == U, route
        assert same(plain, direct), (arrangement, U, args, "no prefix sharing")
    rc, mt, ln, _, msg = O.nw_rows(seqs, 0, len(seqs), *MATRICES[1])
    assert rc == 0, msg
    assert same(direct, mt.astype(np.float64) / ln.astype(np.float64))
