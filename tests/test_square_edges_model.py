"""The numpy side of tests/test_gpu_square_edges.py -- the yardstick, the key blocks and the shard-block builder -- and the tests of it that
need no GPU: the builder against sharding.Plan.locate element by element, the yardstick against a double loop."""
import numpy as np
import pytest

TILE = 128
NOT_AN_ELEMENT = 0xFFFF


def square_model(K, keep, include_diagonal):
    """(hist, (i, j, v)) of a full n x n uint16 key matrix: the histogram of the keys < nbins of the strict upper triangle, and every
    (i, j, K[i, j]) with j > i (j >= i with the diagonal) whose key is < nbins and flagged in keep -- row-major, i.e. sorted by (i, j)"""
    n, nbins = K.shape[0], len(keep)
    i, j = np.triu_indices(n, 1)
    v = K[i, j]
    hist = np.bincount(v[v < nbins], minlength=nbins)
    i, j = np.triu_indices(n, 0 if include_diagonal else 1)
    v = K[i, j]
    ok = v < nbins
    ok[ok] = keep[v[ok]] != 0
    return hist, (i[ok].astype(np.int32), j[ok].astype(np.int32), v[ok])


def keep_mask(rng, nbins, keep0=0):
    """~40 % of the bins kept; nbins - 1 and (nbins >= 3) bin 1 always, bin 2 never, bin 0 as asked"""
    keep = (rng.rand(nbins) < 0.4).astype(np.uint8)
    keep[nbins - 1] = 1
    if nbins >= 3:
        keep[1], keep[2] = 1, 0
    if nbins >= 2:
        keep[0] = keep0
    return keep


def random_keys(rng, shape, nbins):
    """half zeros (counted in a register, not in LDS), keys over [0, nbins + nbins / 8) -- so some are beyond nbins: neither counted nor
    kept --, ~3 % at nbins - 1 and ~3 % at 0xFFFF ("not an element")"""
    hi = min(NOT_AN_ELEMENT, nbins + max(nbins // 8, 3))
    keys = rng.randint(0, hi, shape).astype(np.uint16)
    u = rng.rand(*shape)
    keys[u < 0.5] = 0
    keys[(u >= 0.5) & (u < 0.53)] = nbins - 1
    keys[(u >= 0.53) & (u < 0.56)] = NOT_AN_ELEMENT
    return keys


def hostile_square(rng, n, nbins, keep):
    """an n x n key matrix whose upper triangle is random_keys and whose diagonal and strict lower triangle hold KEPT keys that differ from
    the mirrored upper cell wherever two kept keys exist: reading m[j][i] for m[i][j], or anything at or below the diagonal, changes both the
    histogram and the edges"""
    K = random_keys(rng, (n, n), nbins)
    kept = np.flatnonzero(keep)
    assert len(kept) >= 1
    a, b = int(kept[-1]), int(kept[0])                     # a = nbins - 1; b == a only when a single key is kept
    low = np.where(K.T == a, b, a).astype(np.uint16)
    il = np.tril_indices(n, -1)
    K[il] = low[il]
    K[np.arange(n), np.arange(n)] = a
    return K


def shard_blocks(K, world, fill, tile=TILE):
    """every rank's folded block of K: [world][local_rows][width] uint16, a vectorised restatement of sharding.Plan.locate for all (i, j) with
    j >= tile start of i; every cell locate does not address holds `fill`"""
    from dynaalign_amd.sharding import Plan
    n = K.shape[0]
    plan = Plan(n, 0, world, tile)
    blocks = np.full((world, plan.local_rows, plan.width), fill, np.uint16)
    i = np.arange(n)
    t = i // tile
    q = t // world
    front = q <= plan.local_tiles - 1 - q
    row = np.where(front, q, plan.local_tiles - 1 - q) * tile + i % tile
    rank = t % world
    J = np.broadcast_to(np.arange(n), (n, n))
    start = (t * tile)[:, None]
    valid = J >= start
    col = np.where(front[:, None], J - start, plan.back + J)
    I = np.broadcast_to(i[:, None], (n, n))[valid]
    blocks[rank[I], row[I], col[valid]] = K[valid]
    return plan, blocks


@pytest.mark.parametrize("world", [2, 3])
def test_shard_blocks_is_plan_locate(world):
    from dynaalign_amd.sharding import Plan
    n, fill = 300, 0xABCD
    K = (np.arange(n * n, dtype=np.int64).reshape(n, n) % 40000).astype(np.uint16)           # fill never occurs; neighbours differ
    plan, blocks = shard_blocks(K, world, fill)
    assert blocks.shape == (world, plan.local_rows, plan.width)
    seen = np.zeros(blocks.shape, bool)
    p = Plan(n, 1, world)
    for i in range(n):
        for j in range(i // TILE * TILE, n):
            r, row, col = p.locate(i, j)
            assert blocks[r, row, col] == K[i, j], (i, j)
            assert not seen[r, row, col], ("two elements in one cell", i, j)
            seen[r, row, col] = True
    assert (blocks[~seen] == fill).all() and (~seen).sum() > 0


def test_square_model_is_the_double_loop():
    rng = np.random.RandomState(5)
    n, nbins = 23, 34
    keep = keep_mask(rng, nbins)
    K = hostile_square(rng, n, nbins, keep)
    assert (K >= nbins).any() and (K == NOT_AN_ELEMENT).any() and (K == nbins - 1).any() and (K == 0).any()
    il = np.tril_indices(n, -1)
    assert keep[K[il]].all() and (K[il] != K.T[il]).all() and keep[np.diag(K)].all()
    for diag in (0, 1):
        hist, (ei, ej, ev) = square_model(K, keep, diag)
        want_hist, want = [0] * nbins, []
        for i in range(n):
            for j in range(i, n):
                v = int(K[i, j])
                if j > i and v < nbins:
                    want_hist[v] += 1
                if (j > i or diag) and v < nbins and keep[v]:
                    want.append((i, j, v))
        assert hist.tolist() == want_hist
        assert list(zip(ei.tolist(), ej.tolist(), ev.tolist())) == want
