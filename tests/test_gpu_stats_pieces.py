"""GPU tests of the extrema pass alone (da_dev_upper_extrema on uint16 keys, da_dev_upper_extrema32 on uint32 value ranks) against numpy on
crafted key matrices.  Every comparison is exact.  What the matrices are built to catch:
  * a read outside the mask -- the lower triangle, the diagonal and the padding columns hold keys both below and above every masked key;
  * a wrong tie rule -- the masked keys are drawn from three values, so every extreme occurs many times and only the FIRST column is right;
  * a lost element at an edge -- extremes are planted at column row + 1, at the last column and on either side of every chunk boundary of
    both workgroup shapes (64 x 8 / 256 x 8 keys for uint16, 64 x 4 / 256 x 4 for uint32);
  * the launch shapes -- sizes around one wave's span (1024 masked keys) and the chunk sizes, row strides that keep or break the 16-byte
    alignment of a row, blocks of a larger square with their own origin."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 63, 64, 65, 257, 1024, 1025, 1027, 2051]
NONE = 0xFFFFFFFF
# masked keys (three values), and what surrounds them: below and above all of them
KEYS = {16: (np.uint16, torch.int16, (100, 200, 300), (5, 60000)), 32: (np.uint32, torch.int32, (1000, 70000, 1300000), (3, 0xFFFFFFF0))}
BOUNDARIES = {16: (512, 2048), 32: (256, 1024)}


@pytest.fixture(scope="module")
def device(built):
    from dynaalign_amd import _capi, device
    assert _capi.load().da_device_count() > 0
    return device


def craft(rng, width, rows, ncols, row_begin, col_begin):
    """(rows, ncols) keys of the block rows [row_begin, ...) x columns [col_begin, ...): three-valued inside the mask with planted extremes,
    hostile outside it"""
    dt, _, (lo, mid, hi), (below, above) = KEYS[width]
    K = rng.choice(np.array([lo, mid, hi], dt), size=(rows, ncols), p=(0.2, 0.6, 0.2))
    grow, gcol = row_begin + np.arange(rows)[:, None], col_begin + np.arange(ncols)[None, :]
    mask = gcol > grow
    first = np.maximum(row_begin + np.arange(rows) + 1 - col_begin, 0)             # first masked local column of each row
    plain = [r for r in range(rows) if ncols - first[r] >= 3]
    # rows that are all `mid` with extremes planted: at column row + 1 and again later; at the last column only; around chunk boundaries
    plans = []
    for t, r in enumerate(plain[:: max(len(plain) // 12, 1)]):
        f, last = int(first[r]), ncols - 1
        spots = [(f, last), (last, f), (f, f + 1), (last, last - 1)][t % 4]         # (where hi goes, where lo goes)
        plans.append((r, [spots[0]], [spots[1]]))
    for b in BOUNDARIES[width]:
        for t, r in enumerate([r for r in plain if first[r] < b - 1 and b + 1 < ncols][:6]):
            his = ([b - 1, b], [b], [b - 1], [b, ncols - 1], [b - 1, b + 1], [b])[t]
            los = ([b], [b - 1, b], [b, b + 1], [b - 1], [b], [b + 1, ncols - 1])[t]
            plans.append((r, his, [c for c in los if c not in his]))
    for r, his, los in plans:
        K[r, first[r]:] = mid
        K[r, his] = hi
        K[r, los] = lo
    if len(plain) > 3:                                                              # one row that is a single value: both extremes at its first column
        K[plain[len(plain) // 2], :] = mid
    outside = np.where(rng.rand(rows, ncols) < 0.5, below, above).astype(dt)
    on_diag = gcol == grow
    outside[on_diag] = rng.choice(np.array([below, mid, hi, above], dt), size=int(on_diag.sum()))
    K[~mask] = outside[~mask]
    return K, mask, on_diag


def want_records(K, mask, on_diag, rank=None):
    R = (K if rank is None else rank[K]).astype(np.int64)
    rows = K.shape[0]
    has = mask.any(axis=1)
    lo = np.where(mask, R, 1 << 40)
    hi = np.where(mask, R, -1)
    want = np.zeros((rows, 5), np.int64)
    want[:, 0] = np.where(has, lo.min(axis=1), NONE)
    want[:, 1] = np.where(has, lo.argmin(axis=1), -1)                               # argmin / argmax return the first occurrence
    want[:, 2] = np.where(has, hi.max(axis=1), 0)
    want[:, 3] = np.where(has, hi.argmax(axis=1), -1)
    want[:, 4] = np.where(on_diag.any(axis=1), np.where(on_diag, R, 0).sum(axis=1), NONE)
    return want


def got_records(rec):
    a = rec.cpu().numpy()
    out = a.view(np.uint32).astype(np.int64)
    out[:, 1], out[:, 3] = a[:, 1], a[:, 3]                                         # the columns are signed
    return out


def upload(K, ld, offset, width, rng):
    """the block with leading dimension ld, `offset` elements into an allocation whose every other element is hostile"""
    dt, tdt, _, (below, above) = KEYS[width]
    rows, ncols = K.shape
    host = np.where(rng.rand(rows * ld + offset + 8) < 0.5, below, above).astype(dt)
    np.lib.stride_tricks.as_strided(host[offset:], (rows, ncols), (ld * host.itemsize, host.itemsize))[:] = K
    buf = torch.from_numpy(host.view(np.int16 if width == 16 else np.int32)).cuda()
    return buf, torch.as_strided(buf, (rows, ncols), (ld, 1), offset), host


def layouts(ncols):
    up = -(-ncols // 8) * 8
    return ((ncols, 0), (ncols + 3, 0), (up + 8, 0), (up + 8, 1))                  # ld = n; ld = n + 3; every row aligned; every row misaligned


def run(device, rng, width, n, rows, row_begin, col_begin, ncols, rank=None, tie_case=True):
    K, mask, on_diag = craft(rng, width, rows, ncols, row_begin, col_begin)
    want = want_records(K, mask, on_diag, rank)
    if tie_case and mask.sum() >= 6:
        # the condition the tie cases rest on: each global extreme occurs at least twice in the mask, in at least two different rows
        R = (K if rank is None else rank[K]).astype(np.int64)
        for ext in (R[mask].max(), R[mask].min()):
            hit = mask & (R == ext)
            assert hit.sum() >= 2 and hit.any(axis=1).sum() >= 2, (width, n, rows, row_begin, col_begin)
    rank_t = None if rank is None else torch.from_numpy(rank.view(np.int16)).cuda()
    for ld, offset in layouts(ncols):
        buf, view, host = upload(K, ld, offset, width, rng)
        rec = device.upper_extrema(view, ncols, rank=rank_t, row_begin=row_begin, col_begin=col_begin)
        torch.cuda.synchronize()
        got = got_records(rec)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (width, n, rows, row_begin, col_begin, ld, offset, int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())
        assert np.array_equal(buf.cpu().numpy(), host.view(buf.cpu().numpy().dtype))   # the keys are only read


@pytest.mark.parametrize("width", [16, 32])
@pytest.mark.parametrize("n", SIZES)
def test_the_whole_square_in_one_block(device, n, width):
    rng = np.random.RandomState(1000 * width + n)
    run(device, rng, width, n, n, 0, 0, n)


@pytest.mark.parametrize("width", [16, 32])
@pytest.mark.parametrize("n", SIZES)
def test_blocks_of_the_square_with_their_own_origin(device, n, width):
    """rows [b0, b0 + rows) x columns [b0, n), as the long NW call cuts its problem"""
    rng = np.random.RandomState(2000 * width + n)
    for b0, rows in {(1, 1), (n // 3 + 1, max(n // 4, 1)), (max(n - 9, 1), min(9, n - 1))}:
        if b0 + rows <= n:
            run(device, rng, width, n, rows, b0, b0, n - b0, tie_case=rows >= 4)


@pytest.mark.parametrize("width", [16, 32])
def test_origins_that_put_the_diagonal_outside_the_block_or_leave_rows_empty(device, width):
    rng = np.random.RandomState(77 + width)
    # columns from 5 on: the first five rows have their diagonal element left of the block and every column in the mask
    K, mask, on_diag = craft(rng, width, 40, 300, 0, 5)
    assert mask[:5].all() and not on_diag[:5].any() and on_diag[5:].any(axis=1).all()
    assert (want_records(K, mask, on_diag)[:5, 4] == NONE).all()
    run(device, rng, width, 305, 40, 0, 5, 300)
    # rows from 290 on against columns from 2 on, 300 of them: the mask starts at local column r + 289 and is empty from row 11 on, where the
    # diagonal lies right of the block as well
    K, mask, on_diag = craft(rng, width, 20, 300, 290, 2)
    want = want_records(K, mask, on_diag)
    assert (want[11:, 1] == -1).all() and (want[11:, 3] == -1).all() and (want[12:, 4] == NONE).all() and want[11, 4] != NONE
    run(device, rng, width, 310, 20, 290, 2, 300, tie_case=False)
    # the last row of a square has no element in the mask
    K, mask, on_diag = craft(rng, width, 65, 65, 0, 0)
    assert want_records(K, mask, on_diag)[64].tolist()[:4] == [NONE, -1, 0, -1]


@pytest.mark.parametrize("n", [65, 1027, 2051])
def test_a_rank_table_orders_the_codes_not_their_bits(device, n):
    """uint16 codes compared through a table in which two codes share the top rank -- the smaller code in the EARLIER column, so that a
    comparison of raw keys would pick the later one -- and the largest code has the lowest rank of the mask"""
    lo, mid, hi = KEYS[16][2]
    below, above = KEYS[16][3]
    twin = 150                                                                      # a second code of the top rank, smaller than hi
    rank = np.full(65536, 7, np.uint16)
    rank[[lo, mid, hi, twin, below, above]] = [9, 5, 12, 12, 65535, 0]              # lo (the smallest code) ranks above mid
    bottom = 40000
    rank[bottom] = 2                                                                # a large code with the lowest rank of the mask
    rng = np.random.RandomState(n)
    K, mask, on_diag = craft(rng, 16, n, n, 0, 0)
    rows = [r for r in range(n - 4)][:: max(n // 20, 1)]
    for r in rows:                                                                  # twin before hi, bottom after it; both ranks elsewhere too
        span = n - (r + 1)
        K[r, r + 1 + span // 3] = twin
        K[r, r + 1 + span // 2 + 1] = hi
        K[r, n - 1] = bottom
    R = rank[K].astype(np.int64)
    want = want_records(K, mask, on_diag, rank)
    for r in rows:
        first_top = int(np.nonzero(mask[r] & (R[r] == 12))[0][0])
        assert want[r, 2] == 12 and want[r, 3] == first_top and K[r, first_top] in (twin, hi)
        assert want[r, 0] == 2 and K[r, want[r, 1]] == bottom
    assert any(K[r, want[r, 3]] == twin for r in rows)                              # somewhere the first of the top rank is the smaller code
    rank_t = torch.from_numpy(rank.view(np.int16)).cuda()
    for ld, offset in layouts(n):
        buf, view, host = upload(K, ld, offset, 16, rng)
        got = got_records(device.upper_extrema(view, n, rank=rank_t))
        assert np.array_equal(got, want), (n, ld, offset, np.nonzero((got != want).any(axis=1))[0][:3])


def test_nothing_is_written_beyond_the_records_and_no_rows_is_no_launch(device):
    from dynaalign_amd import _capi
    lib = _capi.load()
    rng = np.random.RandomState(3)
    stream = torch.cuda.current_stream().cuda_stream
    for width in (16, 32):
        K, mask, on_diag = craft(rng, width, 70, 1500, 0, 0)
        buf, view, host = upload(K, 1504, 0, width, rng)
        rec = torch.full((70 * 5 + 16,), -7, dtype=torch.int32, device="cuda")
        if width == 16:
            _capi.check(lib.da_dev_upper_extrema(view.data_ptr(), 70, 1500, 1504, None, 0, 0, rec.data_ptr(), stream))
            _capi.check(lib.da_dev_upper_extrema(view.data_ptr(), 0, 1500, 1504, None, 0, 0, rec.data_ptr() + 70 * 20, stream))
        else:
            _capi.check(lib.da_dev_upper_extrema32(view.data_ptr(), 70, 1500, 1504, 0, 0, rec.data_ptr(), stream))
            _capi.check(lib.da_dev_upper_extrema32(view.data_ptr(), 0, 1500, 1504, 0, 0, rec.data_ptr() + 70 * 20, stream))
        torch.cuda.synchronize()
        assert bool((rec[70 * 5:] == -7).all())
        assert np.array_equal(got_records(rec[:70 * 5].view(70, 5)), want_records(K, mask, on_diag))
