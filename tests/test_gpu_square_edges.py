"""GPU tests of the square threshold kernels k_upper_histogram / k_extract_edges (csrc/graph_kernels.hip) on key matrices built here, in the
three layouts they read: dense (da_dev_upper_histogram, da_dev_extract_edges), through a row map (da_dev_*_rows) and one rank's folded shard
block (da_dev_shard_*).  The yardstick is numpy on the full n x n key matrix (test_square_edges_model.square_model); every comparison is exact.
The C entry points are called with buffers owned here, 64 guard slots behind the capacity; edge lists are compared after a sort by (i, j) --
tiles reserve their slots with one atomic each, so the order between tiles is not defined.

What the key matrices are built to catch: the strict lower triangle and the diagonal hold KEPT keys that differ from the mirrored upper cell
(a read of the wrong side changes histogram and edges), keys at nbins - 1, keys beyond nbins and 0xFFFF cells (neither counted nor kept),
odd leading dimensions and unaligned bases (the 2-byte loads of interior tiles), nbins on both sides of the LDS histogram's 8192 bins, and
shard blocks whose every unaddressed cell holds a kept key."""
import time

import numpy as np
import pytest
import torch

from test_gpu_cross import strided
from test_gpu_cross_edges import layouts
from test_square_edges_model import NOT_AN_ELEMENT, TILE, hostile_square, keep_mask, random_keys, shard_blocks, square_model

pytestmark = pytest.mark.gpu

GUARD = 64


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    from dynaalign_amd import _capi
    assert _capi.load().da_device_count() > 0
    return dynaalign_amd


def stream():
    return torch.cuda.current_stream().cuda_stream


class Source:
    """a key matrix on the device in one layout, and the two C calls that read it"""

    def __init__(self, keys, n, ld, offset, uidx=None, rank=0, world=0):
        from dynaalign_amd import _capi
        self.lib = _capi.load()
        self.n, self.ld, self.offset, self.rank, self.world = n, ld, offset, rank, world
        self.buf, self.view = strided(keys.shape[0], keys.shape[1], ld, torch.int16, offset)
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(keys).view(np.int16)).cuda())
        self.uidx = None if uidx is None else torch.from_numpy(np.ascontiguousarray(uidx, np.int32)).cuda()
        self.what = (keys.shape, n, ld, offset, "rows" if uidx is not None else "shard %d/%d" % (rank, world) if world else "dense")

    def hist_call(self, nbins, d_hist):
        p = self.view.data_ptr()
        if self.uidx is not None:
            return self.lib.da_dev_upper_histogram_rows(p, self.ld, self.uidx.data_ptr(), self.n, nbins, d_hist, stream())
        if self.world:
            return self.lib.da_dev_shard_histogram(p, self.ld, self.n, self.rank, self.world, nbins, d_hist, stream())
        return self.lib.da_dev_upper_histogram(p, self.ld, self.n, nbins, d_hist, stream())

    def extract_call(self, d_keep, nbins, diag, d_i, d_j, d_v, capacity, d_count):
        p = self.view.data_ptr()
        if self.uidx is not None:
            return self.lib.da_dev_extract_edges_rows(p, self.ld, self.uidx.data_ptr(), self.n, d_keep, nbins, diag, d_i, d_j, d_v, capacity,
                                                      d_count, stream())
        if self.world:
            return self.lib.da_dev_shard_extract_edges(p, self.ld, self.n, self.rank, self.world, d_keep, nbins, diag, d_i, d_j, d_v, capacity,
                                                       d_count, stream())
        return self.lib.da_dev_extract_edges(p, self.ld, self.n, d_keep, nbins, diag, d_i, d_j, d_v, capacity, d_count, stream())

    def assert_only_read(self):
        """the sentinel fill around and between the rows of the matrix is intact"""
        pad = torch.ones(self.buf.numel(), dtype=torch.bool, device="cuda")
        torch.as_strided(pad, tuple(self.view.shape), (self.ld, 1), self.offset).fill_(False)
        assert bool((self.buf[pad] == -7).all()), ("the source was written",) + self.what


class Edges:
    """sentinel-filled output buffers of `slots` entries and the counter"""

    def __init__(self, slots, count=0):
        self.i = torch.full((slots,), -7, dtype=torch.int32, device="cuda")
        self.j = torch.full((slots,), -7, dtype=torch.int32, device="cuda")
        self.v = torch.full((slots,), -7, dtype=torch.int16, device="cuda")
        self.count = torch.full((1,), count, dtype=torch.int64, device="cuda")

    def host(self):
        torch.cuda.synchronize()
        return int(self.count.item()), self.i.cpu().numpy(), self.j.cpu().numpy(), self.v.cpu().numpy().view(np.uint16)

    def untouched_from(self, first):
        return bool((self.i[first:] == -7).all()) and bool((self.j[first:] == -7).all()) and bool((self.v[first:] == -7).all())


def histogram(src, nbins, hist=None):
    from dynaalign_amd import _capi
    if hist is None:
        hist = torch.zeros(nbins, dtype=torch.int64, device="cuda")
    _capi.check(src.hist_call(nbins, hist.data_ptr()))
    return hist


def extract(src, keep, diag, capacity, out):
    from dynaalign_amd import _capi
    keep_t = torch.from_numpy(np.ascontiguousarray(keep, np.uint8)).cuda()
    _capi.check(src.extract_call(keep_t.data_ptr(), len(keep), diag, out.i.data_ptr(), out.j.data_ptr(), out.v.data_ptr(), capacity,
                                 out.count.data_ptr()))
    return out.host()


def by_position(i, j, v):
    order = np.lexsort((j, i))
    return np.stack([np.asarray(i, np.int64)[order], np.asarray(j, np.int64)[order], np.asarray(v, np.int64)[order]], 1)


def triples(n, i, j, v):
    """one int64 per (i, j, v)"""
    return (np.asarray(i, np.int64) * n + np.asarray(j, np.int64)) * 65536 + np.asarray(v, np.int64)


def check(src, keep, model):
    """histogram and, with and without the diagonal, the edge list of one source against the model; nothing behind the capacity is written"""
    nbins = len(keep)
    hist = histogram(src, nbins).cpu().numpy()
    assert np.array_equal(hist, model[0][0]), ("histogram",) + src.what
    got = {}
    for diag in (0, 1):
        wi, wj, wv = model[diag][1]
        total = len(wi)
        out = Edges(total + GUARD)
        count, i, j, v = extract(src, keep, diag, total, out)
        assert count == total, ("edge count", diag, count, total) + src.what
        got[diag] = by_position(i[:total], j[:total], v[:total])
        assert np.array_equal(got[diag], by_position(wi, wj, wv)), ("edges", diag) + src.what
        assert out.untouched_from(total), ("written beyond the capacity", diag) + src.what
    src.assert_only_read()
    return hist, got


def models(K, keep):
    return square_model(K, keep, 0), square_model(K, keep, 1)


# ---- dense layout -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 127, 128, 129, 255, 256, 257, 385])
def test_dense_tile_edges_in_every_layout(da, n):
    rng = np.random.RandomState(n)
    nbins = 501
    keep = keep_mask(rng, nbins)
    K = hostile_square(rng, n, nbins, keep)
    model = models(K, keep)
    if n >= 127:
        up = K[np.triu_indices(n, 1)]
        assert (up >= nbins).any() and (up == NOT_AN_ELEMENT).any() and (up == nbins - 1).any() and (up == 0).mean() > 0.4
        assert 0 < len(model[0][1][0]) < len(up)
    if n == 1:
        assert model[0][0].sum() == 0 and len(model[0][1][0]) == 0 and len(model[1][1][0]) == 1
    for ld, offset in layouts(n):
        check(Source(K, n, ld, offset), keep, model)
    keep = keep_mask(rng, nbins, keep0=1)                   # zeros kept: most of the triangle is an edge
    K = hostile_square(rng, n, nbins, keep)
    model = models(K, keep)
    for ld, offset in (layouts(n)[0], layouts(n)[4]):
        check(Source(K, n, ld, offset), keep, model)


def test_dense_bin_counts_on_both_sides_of_the_lds_split(da):
    n = 257
    sides = set()
    for nbins in (1, 34, 501, 8192, 8193, 65535):
        rng = np.random.RandomState(nbins)
        keep = keep_mask(rng, nbins)
        K = hostile_square(rng, n, nbins, keep)
        model = models(K, keep)
        sides.add(nbins <= 8192)
        if nbins > 8192:
            assert model[0][0][8192:].sum() > 0 and keep[8192:].any()
        if nbins < 65535:
            assert (K[np.triu_indices(n, 1)] >= nbins).any()
        for ld, offset in layouts(n):
            check(Source(K, n, ld, offset), keep, model)
    assert sides == {True, False}


def test_65536_bins_are_refused_and_nothing_is_touched(da):
    """the entry checks admit nbins = 65536, the launcher refuses it: key 65535 stands for "not an element" """
    from dynaalign_amd import _capi
    n = 257
    rng = np.random.RandomState(3)
    keep = np.ones(65536, np.uint8)
    K = random_keys(rng, (n, n), 65535)
    plan, blocks = shard_blocks(K, 2, 7)
    sources = [Source(K, n, n, 1), Source(K, n, n + 7, 0, uidx=np.arange(n)), Source(blocks[1], n, plan.width, 0, rank=1, world=2)]
    for src in sources:
        hist = torch.full((65536,), 7, dtype=torch.int64, device="cuda")
        with pytest.raises(_capi.DynaAlignError, match="value 65535 is reserved") as e:
            histogram(src, 65536, hist)
        assert e.value.code == _capi.DA_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert bool((hist == 7).all()), src.what
        out = Edges(GUARD, count=7)
        with pytest.raises(_capi.DynaAlignError, match="value 65535 is reserved") as e:
            extract(src, keep, 1, GUARD, out)
        assert e.value.code == _capi.DA_ERR_UNSUPPORTED
        assert out.host()[0] == 7 and out.untouched_from(0), src.what
        src.assert_only_read()


def test_dense_calls_accumulate(da):
    """the caller zeroes d_hist and *d_count: a second call adds to the histogram and appends to the list"""
    n, nbins = 257, 501
    rng = np.random.RandomState(8)
    keep = keep_mask(rng, nbins)
    K = hostile_square(rng, n, nbins, keep)
    model = models(K, keep)
    src = Source(K, n, n, 1)
    hist = histogram(src, nbins)
    histogram(src, nbins, hist)
    assert np.array_equal(hist.cpu().numpy(), 2 * model[0][0])
    wi, wj, wv = model[1][1]
    total = len(wi)
    out = Edges(2 * total + GUARD)
    assert extract(src, keep, 1, 2 * total, out)[0] == total
    count, i, j, v = extract(src, keep, 1, 2 * total, out)
    assert count == 2 * total and out.untouched_from(2 * total)
    want = by_position(np.repeat(wi, 2), np.repeat(wj, 2), np.repeat(wv, 2))
    assert np.array_equal(by_position(i[:count], j[:count], v[:count]), want)


@pytest.mark.parametrize("ld,offset", [(264, 0), (257, 1)])
def test_dense_short_capacity_counts_everything_and_stores_no_more(da, ld, offset):
    n, nbins = 257, 501
    rng = np.random.RandomState(9)
    keep = keep_mask(rng, nbins)
    K = hostile_square(rng, n, nbins, keep)
    wi, wj, wv = square_model(K, keep, 1)[1]
    total = len(wi)
    assert total > 1000
    want = triples(n, wi, wj, wv)
    src = Source(K, n, ld, offset)
    for capacity in (0, total - 5, total):
        out = Edges(capacity + GUARD)
        count, i, j, v = extract(src, keep, 1, capacity, out)
        assert count == total, capacity
        assert out.untouched_from(capacity), ("written at or beyond the capacity", capacity)
        stored = triples(n, i[:capacity], j[:capacity], v[:capacity])
        assert len(np.unique(stored)) == capacity and np.isin(stored, want).all(), capacity


def test_dense_more_tiles_than_the_grid_cap(da):
    """n = 11 600: 91 tile rows, 4186 upper tiles > the 4096 workgroups k_upper_histogram is launched with -- its L += gridDim.x loop runs a
    second time in the first 90 workgroups.  ~97 % zeros, the rest in 1 .. 500; the numpy side works in row blocks on the non-zero cells"""
    t0 = time.perf_counter()
    n, nbins = 11600, 501
    T = -(-n // TILE)
    assert T * (T + 1) // 2 == 4186 > 256 * 16
    rng = np.random.RandomState(116)
    K = np.zeros((n, n), np.uint16)
    cells = rng.randint(0, n * n, int(0.03 * n * n))
    K.ravel()[cells] = rng.randint(1, nbins, len(cells))
    keep = np.zeros(nbins, np.uint8)
    keep[[7, 500]] = 1
    hist = np.zeros(nbins, np.int64)
    edges, late = [], 0
    for r0 in range(0, n, 1024):
        block = K[r0:r0 + 1024]
        bi, bj = np.nonzero(block)
        v = block[bi, bj]
        bi = bi + r0
        hist += np.bincount(v[bj > bi], minlength=nbins)
        late += int(((bj > bi) & (bi >= 79 * TILE)).sum())
        sel = (bj >= bi) & (keep[v] != 0)
        edges.append((bi[sel], bj[sel], v[sel]))
    hist[0] = n * (n - 1) // 2 - hist.sum()
    wi, wj, wv = (np.concatenate(part) for part in zip(*edges))
    total = len(wi)
    assert 0.96 < hist[0] / (n * (n - 1) // 2) < 0.98 and 2000 < total < 20000
    assert 79 * T - 79 * 78 // 2 >= 256 * 16                # tile rows 79 .. 90 are reached only by the second trip of the loop ...
    assert hist[1:].sum() > 10 ** 6 and late > 10000       # ... and hold counts the histogram would miss without it
    t1 = time.perf_counter()
    src = Source(K, n, n, 0)
    assert src.view.data_ptr() % 16 == 0 and src.ld % 8 == 0
    got = histogram(src, nbins).cpu().numpy()
    out = Edges(total + GUARD)
    count, i, j, v = extract(src, keep, 1, total, out)
    t2 = time.perf_counter()
    assert np.array_equal(got, hist)
    assert count == total and out.untouched_from(total)
    assert np.array_equal(by_position(i[:total], j[:total], v[:total]), by_position(wi, wj, wv))
    print("n = 11600: host side %.2f s, upload + device calls %.2f s, compare %.2f s" % (t1 - t0, t2 - t1, time.perf_counter() - t2))


# ---- through a row map ------------------------------------------------------------------------------------------------------------------

def row_maps(rng, n):
    """(rows in the table, map): one row for all; two; 40 with repeats; the identity; the reversed order"""
    return [(1, np.zeros(n, np.int32)), (2, rng.randint(0, 2, n).astype(np.int32)), (40, rng.randint(0, 40, n).astype(np.int32)),
            (n, np.arange(n, dtype=np.int32)), (n, np.arange(n - 1, -1, -1, dtype=np.int32))]


@pytest.mark.parametrize("n", [129, 257, 385])
def test_row_map_is_the_materialised_matrix(da, n):
    rng = np.random.RandomState(1000 + n)
    nbins = 501
    keep = keep_mask(rng, nbins)
    for U, uidx in row_maps(rng, n):
        if U == n and uidx[0] == 0:
            rows = hostile_square(rng, n, nbins, keep)      # the identity map: the dense matrix itself
        else:
            rows = random_keys(rng, (U, n), nbins)
            rows[rng.rand(U, n) < 0.2] = nbins - 1          # kept keys on both sides of the diagonal, not mirrored
        assert 0 <= uidx.min() and uidx.max() == U - 1 and (U >= n or len(np.unique(uidx)) < n)
        M = rows[uidx]
        assert (M != M.T).mean() > 0.3
        model = models(M, keep)
        dense = check(Source(M, n, -(-n // 8) * 8, 0), keep, model)
        for ld, offset in layouts(n):
            got = check(Source(rows, n, ld, offset, uidx=uidx), keep, model)
            assert np.array_equal(got[0], dense[0]) and all(np.array_equal(got[1][d], dense[1][d]) for d in (0, 1))


# ---- one rank's folded shard block ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [100, 129, 700, 1025])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_shard_blocks_with_hostile_padding(da, world, n):
    """the ranks' histograms sum to the histogram of the matrix, their edge lists are disjoint and their union is its edge set -- on blocks
    whose every cell Plan.locate does not address (columns left of a front row's diagonal tile, columns beyond n, tile rows beyond the
    last) holds a kept key"""
    from dynaalign_amd.sharding import Plan
    rng = np.random.RandomState(77 * world + n)
    nbins = 501
    keep = keep_mask(rng, nbins)
    K = hostile_square(rng, n, nbins, keep)
    model = models(K, keep)
    plan, blocks = shard_blocks(K, world, nbins - 1)
    addressed = sum(n - i // TILE * TILE for i in range(n))
    assert keep[nbins - 1] and blocks.size - addressed >= TILE * TILE          # the padding, all of it a kept key
    idle = [r for r in range(world) if not Plan(n, r, world).my_rows()]
    if (world, n) == (8, 100):
        assert idle == list(range(1, 8))
    for ld, offset in ((plan.width, 0), (plan.width + 8, 0), (plan.width + 9, 3)):
        hist = np.zeros(nbins, np.int64)
        lists = {0: [], 1: []}
        for rank in range(world):
            src = Source(blocks[rank], n, ld, offset, rank=rank, world=world)
            mine = histogram(src, nbins).cpu().numpy()
            hist += mine
            for diag in (0, 1):
                out = Edges(len(model[diag][1][0]) + GUARD)
                count, i, j, v = extract(src, keep, diag, len(model[diag][1][0]), out)
                assert out.untouched_from(count), src.what
                lists[diag].append((i[:count], j[:count], v[:count]))
                if rank in idle:
                    assert count == 0 and mine.sum() == 0, src.what
                else:
                    assert ((i[:count] // TILE) % world == rank).all(), src.what
            src.assert_only_read()
        assert np.array_equal(hist, model[0][0]), (world, n, ld, offset)
        for diag in (0, 1):
            i, j, v = (np.concatenate(part) for part in zip(*lists[diag]))
            pairs = np.asarray(i, np.int64) * n + j
            assert len(np.unique(pairs)) == len(pairs), ("the ranks' lists overlap", world, n, ld, offset, diag)
            assert np.array_equal(by_position(i, j, v), by_position(*model[diag][1])), (world, n, ld, offset, diag)
