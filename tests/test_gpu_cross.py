"""GPU tests of the two-set calls: similarityMH_cross / similarityNW_cross on the host boundary (both output layouts), the one-call device
route (direct and duplicate-collapsing), the rectangle calls da_dev_mh_compare_rect / da_dev_nw_rect on operands built here, and
MinHashSession.cross.  Every expected value is a block of what the oracle computes on the concatenation c(x, y): rows [0, m), columns
[m, m + n).  All comparisons are bit for bit (float64 as uint64, the NaN pattern included)."""
import os

import numpy as np
import pytest
import torch

import oracle_lib as O

pytestmark = pytest.mark.gpu

SEED = 12345
AA24 = "ARNDCQEGHILKMFPSTWYVBZX*"


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    from dynaalign_amd import _capi
    assert _capi.load().da_device_count() > 0
    return dynaalign_amd


class switches:
    """DYNAALIGN_* switches for the duration of a block (the Python mirror reloads the library's configuration when they change)"""

    def __init__(self, **kw):
        self.kw = {k: str(v) for k, v in kw.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def two_sets(rng, m, n, alphabet, lo=0, hi=31, high_bytes=False):
    """strings of length lo..hi-1: some shorter than any k, some empty, some byte-identical within a side and across the sides"""
    def mk():
        s = "".join(alphabet[i] for i in rng.randint(0, len(alphabet), rng.randint(lo, hi)))
        if high_bytes and s and rng.randint(0, 4) == 0:
            s = s[:-1] + chr(0x80 + rng.randint(0, 128))
        return s
    pool = [mk() for _ in range(max(2, (m + n) // 3))] + ["", "A", "AC"]
    draw = lambda cnt: [pool[rng.randint(0, len(pool))] if rng.randint(0, 3) else mk() for _ in range(cnt)]
    x, y = draw(m), draw(n)
    if m > 1 and n > 1:
        y[-1] = x[0]                    # one string certainly on both sides
        x[-1] = x[0]                    # ... and twice in x
    return x, y


def strided(rows, cols, ld, dtype, offset_elems):
    """a (rows, cols) device view with leading dimension ld whose first element sits offset_elems elements into its allocation"""
    buf = torch.full((rows * ld + offset_elems + 8,), -7, dtype=dtype, device="cuda")
    return buf, torch.as_strided(buf, (rows, cols), (ld, 1), offset_elems)


def host_cross_mh(x, y, k, n_hash, seeds, column_major):
    from dynaalign_amd import _capi
    lib = _capi.load()
    xr, xo = O.pack(x)
    yr, yo = O.pack(y)
    m, n = len(x), len(y)
    out = np.full(m * n, -7.0)
    _capi.check(lib.da_similarity_mh_cross(xr.ctypes.data, xo.ctypes.data, m, yr.ctypes.data, yo.ctypes.data, n, k, n_hash,
                                           np.ascontiguousarray(seeds, np.uint32).ctypes.data, out.ctypes.data, column_major))
    return out.reshape((n, m) if column_major else (m, n))


def host_cross_nw(x, y, matrix, go, ge, column_major):
    from dynaalign_amd import _capi
    lib = _capi.load()
    xr, xo = O.pack(x)
    yr, yo = O.pack(y)
    m, n = len(x), len(y)
    out = np.full(m * n, -7.0)
    _capi.check(lib.da_similarity_nw_cross(xr.ctypes.data, xo.ctypes.data, m, yr.ctypes.data, yo.ctypes.data, n, matrix.encode(), go, ge,
                                           out.ctypes.data, column_major))
    return out.reshape((n, m) if column_major else (m, n))


def device_sets(x, y):
    from dynaalign_amd import device
    return (device.DeviceSequences(*O.pack(x)), device.DeviceSequences(*O.pack(y)), device.DeviceSequences(*O.pack(x + y)))


def padded_operand(sig_xy, m, n, n_hash):
    """[x ; filler ; y] with x padded to a multiple of 128 rows, coded by ONE dictionary run: what makes the rectangle's origins tile-aligned"""
    from dynaalign_amd import device
    m_pad = -(-m // 128) * 128
    joint = torch.empty((m_pad + n, sig_xy.shape[1]), dtype=torch.int32, device="cuda")
    joint[:m] = sig_xy[:m]
    if m_pad > m:
        joint[m:m_pad] = sig_xy[torch.arange(m_pad - m, device="cuda") % m]
    joint[m_pad:] = sig_xy[m:m + n]
    return device.mh_planes(joint, m_pad + n, n_hash), m_pad


def check_mh_shape(da, m, n, k, n_hash, rng, odd_ld=False):
    from dynaalign_amd import device, _capi
    x, y = two_sets(rng, m, n, "ACDEFGHIKLMNPQRSTVWY", high_bytes=True)
    seeds = O.seeds(SEED, n_hash)
    rc, full = O.similarity_mh(x + y, k, n_hash, seeds)
    assert rc == 0
    want = full[:m, m:]
    want_cnt = O.mh_counts(O.signatures(x + y, k, n_hash, seeds), 0, m)[:, m:]
    # host boundary: the Python mirror, both layouts of the C call
    got = da.similarityMH_cross(x, y, k, n_hash, seed=SEED)
    assert same(got, want), ("mirror", m, n, k, n_hash)
    assert got.dimnames == [[str(i + 1) for i in range(m)], [str(j + 1) for j in range(n)]]
    rm, cm = host_cross_mh(x, y, k, n_hash, seeds, 0), host_cross_mh(x, y, k, n_hash, seeds, 1)
    assert same(rm, want) and same(cm, rm.T), ("host", m, n, k, n_hash)
    # one-call device route
    dx, dy, dxy = device_sets(x, y)
    for min_n in ("999999", "1"):                                  # direct; duplicate route admitted whatever the counts
        with switches(DYNAALIGN_MH_DEDUP_MIN_N=min_n, DYNAALIGN_MH_DEDUP_MAX_PCT=100):
            out = device.similarity_mh_cross(dx, dy, k, n_hash, seeds)
            torch.cuda.synchronize()
            route = device.mh_cross_last_route()
        assert same(out.cpu().numpy(), want), ("one call", min_n, m, n, k, n_hash, route)
        assert (route["m"], route["n"]) == (m, n)
        if min_n == "1" and (n % 2 == 0) and any(x) and any(y):   # the rectangular expansion takes even ld; all-empty sides have nothing to plan
            assert route["dedup"] and route["unique_x"] == len(set(x)) and route["unique_y"] == len(set(y)), route
        if min_n != "1":
            assert not route["dedup"]
    if n % 2 == 1 and any(x) and any(y):                           # odd n in an even ld: the duplicate route, its last column peeled by the expansion
        buf, view = strided(m, n, n + 1, torch.float64, 0)
        with switches(DYNAALIGN_MH_DEDUP_MIN_N=1, DYNAALIGN_MH_DEDUP_MAX_PCT=100):
            device.similarity_mh_cross(dx, dy, k, n_hash, seeds, out=view)
            torch.cuda.synchronize()
            route = device.mh_cross_last_route()
        assert route["dedup"] and route["unique_x"] == len(set(x)) and route["unique_y"] == len(set(y)), route
        assert same(view.cpu().numpy(), want), ("one call, odd n in an even ld", m, n)
        assert int((buf != -7).sum().item()) <= m * n
    if odd_ld:                                                     # odd ld + an output 8 bytes into its allocation: the direct route, compiled stores
        buf, view = strided(m, n, n + 1 + (n % 2), torch.float64, 1)
        with switches(DYNAALIGN_MH_DEDUP_MIN_N=1, DYNAALIGN_MH_DEDUP_MAX_PCT=100):
            device.similarity_mh_cross(dx, dy, k, n_hash, seeds, out=view)
            torch.cuda.synchronize()
            assert not device.mh_cross_last_route()["dedup"]
        assert same(view.cpu().numpy(), want)
    # the rectangle call on operands built here: c(x, y) as it is (col_begin = m: a multiple of 128 only when m is) and the padded one
    sig, planes = device.minhash_signatures(dxy, k, n_hash, seeds)
    pplanes, m_pad = padded_operand(sig, m, n, n_hash)
    for P, N, c0 in ((planes, m + n, m), (pplanes, m_pad + n, m_pad)):
        f = device.mh_compare_rect(P, N, n_hash, 0, m, c0, c0 + n, _capi.DA_OUT_F64)
        c = device.mh_compare_rect(P, N, n_hash, 0, m, c0, c0 + n, _capi.DA_OUT_COMPACT)
        assert same(f.cpu().numpy(), want), ("rect f64", m, n, c0)
        assert np.array_equal(c.cpu().numpy().view(np.uint16), want_cnt), ("rect u16", m, n, c0)
        # the transposed rectangle (rows of y, columns of x) is the transpose
        t = device.mh_compare_rect(P, N, n_hash, c0, c0 + n, 0, m, _capi.DA_OUT_F64)
        assert same(t.cpu().numpy(), want.T), ("rect transposed", m, n, c0)
        if odd_ld:
            for dt, kind, off, exp in ((torch.float64, _capi.DA_OUT_F64, 1, want), (torch.int16, _capi.DA_OUT_COMPACT, 4, want_cnt)):
                for ld in (n + 1 - (n % 2), n + 2 - (n % 2)):      # odd, then even: unaligned either way
                    buf, view = strided(m, n, ld, dt, off)
                    device.mh_compare_rect(P, N, n_hash, 0, m, c0, c0 + n, kind, out=view)
                    g = view.cpu().numpy()
                    assert same(g, exp) if kind == _capi.DA_OUT_F64 else np.array_equal(g.view(np.uint16), exp), ("rect strided", m, n, ld)
                    assert int((buf != -7).sum().item()) <= m * n   # nothing outside the rectangle was written
    # a sub-rectangle with odd origins, and a rectangle across the global diagonal of the operand (its elements keep the forced n_hash)
    if m >= 3 and n >= 3:
        sub = device.mh_compare_rect(planes, m + n, n_hash, 1, m - 1, m + 1, m + n - 1, _capi.DA_OUT_F64)
        assert same(sub.cpu().numpy(), want[1:m - 1, 1:n - 1])
    sq = device.mh_compare_rect(planes, m + n, n_hash, 0, m + n, 0, m + n, _capi.DA_OUT_F64)
    assert same(sq.cpu().numpy(), full)


SHAPES = [(m, n) for m in (1, 3, 127, 128, 129, 200) for n in (1, 2, 128, 130, 257)]


@pytest.mark.parametrize("m,n", SHAPES)
def test_minhash_small_shapes_against_the_oracle(da, m, n):
    i = SHAPES.index((m, n))
    rng = np.random.RandomState(100 + i)
    k, n_hash = (1, 2, 4, 5)[i % 4], (8, 50, 500, 600)[(i // 4 + i) % 4]
    check_mh_shape(da, m, n, k, n_hash, rng, odd_ld=(i % 3 == 0))


@pytest.mark.parametrize("env", [{"DYNAALIGN_PLANE_BITS": 16}, {"DYNAALIGN_PLANE_BITS": 32}, {"DYNAALIGN_K2_NO_ASM": 1}, {"DYNAALIGN_PLANE_BITS": 14},
                                 {"DYNAALIGN_NO_HOST_WIDEN": 1}])
@pytest.mark.parametrize("m,n,k,n_hash", [(200, 257, 4, 500), (128, 128, 2, 50), (129, 130, 5, 600), (3, 2, 1, 8)])
def test_minhash_plane_counts_and_the_compiled_kernel(da, env, m, n, k, n_hash):
    rng = np.random.RandomState(7 * m + n)
    with switches(**env):
        check_mh_shape(da, m, n, k, n_hash, rng, odd_ld=True)


def test_minhash_no_forced_diagonal_and_short_strings(da):
    """R[i][i] is whatever the signatures say; strings shorter than k hash as themselves, so two of them agree everywhere"""
    x, y = ["ACDEFGHIK", "AC", "", "WWWWWWWW"], ["QQQQQQQQ", "AC", "", "ACDEFGHIK", "A"]
    got = da.similarityMH_cross(x, y, 4, 50, seed=SEED)
    want = O.similarity_mh(x + y, 4, 50, O.seeds(SEED, 50))[1][:4, 4:]
    assert same(got, want)
    assert got[0, 0] != 1.0 and got[0, 3] == 1.0 and got[1, 1] == 1.0 and got[2, 2] == 1.0


NW_CASES = [("BLOSUM62", 10, 4), ("BLOSUM45", 0, 0), ("BLOSUM80", 5, 0), ("BLOSUM100", 0, 3), ("BLOSUM50", 11, 1)]


def nw_expected(x, y, matrix, go, ge):
    m = len(x)
    rc, full, _ = O.similarity_nw(x + y, matrix, go, ge)
    assert rc == 0
    rc, nm, ln, _, _ = O.nw_rows(x + y, 0, m, matrix, go, ge)
    assert rc == 0
    return full[:m, m:], ((nm << 8) | (ln & 255)).astype(np.uint16)[:, m:], nm[:, m:], ln[:, m:]


@pytest.mark.parametrize("m,n", SHAPES)
def test_nw_small_shapes_against_the_oracle(da, m, n):
    from dynaalign_amd import device, _capi
    i = SHAPES.index((m, n))
    rng = np.random.RandomState(300 + i)
    matrix, go, ge = NW_CASES[i % len(NW_CASES)]
    x, y = two_sets(rng, m, n, AA24)
    want, want_code, _, _ = nw_expected(x, y, matrix, go, ge)
    got = da.similarityNW_cross(x, y, matrix, go, ge)
    assert same(got, want), ("mirror", m, n, matrix, go, ge)
    rm, cm = host_cross_nw(x, y, matrix, go, ge, 0), host_cross_nw(x, y, matrix, go, ge, 1)
    assert same(rm, want) and same(cm, rm.T)
    with switches(DYNAALIGN_NO_HOST_WIDEN=1):
        assert same(host_cross_nw(x, y, matrix, go, ge, 0), want) and same(host_cross_nw(x, y, matrix, go, ge, 1), want.T)
    if any(not a for a in x) and any(not b for b in y):
        assert np.isnan(want).any()                                  # both empty: 0 / 0
    # the rectangle call on the codes of c(x, y): rows of x against columns of y, and rows of y against columns of x
    _, _, dxy = device_sets(x, y)
    assert int(device.nw_encode(dxy).item()) == 0
    f = device.nw_rect(dxy, matrix, go, ge, 0, m, m, m + n, _capi.DA_OUT_F64)
    c = device.nw_rect(dxy, matrix, go, ge, 0, m, m, m + n, _capi.DA_OUT_COMPACT)
    t = device.nw_rect(dxy, matrix, go, ge, m, m + n, 0, m, _capi.DA_OUT_F64)
    tc = device.nw_rect(dxy, matrix, go, ge, m, m + n, 0, m, _capi.DA_OUT_COMPACT)
    assert same(f.cpu().numpy(), want) and same(t.cpu().numpy(), want.T)
    assert np.array_equal(c.cpu().numpy().view(np.uint16), want_code) and np.array_equal(tc.cpu().numpy().view(np.uint16), want_code.T)
    if i % 3 == 0:
        for dt, kind, off, exp in ((torch.float64, _capi.DA_OUT_F64, 1, want), (torch.int16, _capi.DA_OUT_COMPACT, 4, want_code)):
            buf, view = strided(m, n, n + 1 - (n % 2), dt, off)
            device.nw_rect(dxy, matrix, go, ge, 0, m, m, m + n, kind, out=view)
            g = view.cpu().numpy()
            assert same(g, exp) if kind == _capi.DA_OUT_F64 else np.array_equal(g.view(np.uint16), exp)
            assert int((buf != -7).sum().item()) <= m * n
    if m >= 3 and n >= 3:
        sub = device.nw_rect(dxy, matrix, go, ge, 1, m - 1, m + 1, m + n - 1, _capi.DA_OUT_F64)
        assert same(sub.cpu().numpy(), want[1:m - 1, 1:n - 1])
    # a rectangle across the diagonal of c(x, y): element (i, j) is calc(seq[min], seq[max]), as da_dev_nw's row blocks
    rc, full, _ = O.similarity_nw(x + y, matrix, go, ge)
    lo, hi = max(0, m - 2), min(m + n, m + 3)
    blk = device.nw_rect(dxy, matrix, go, ge, lo, hi, 0, m + n, _capi.DA_OUT_F64)
    assert same(blk.cpu().numpy(), full[lo:hi])


def test_nw_longer_sequences_take_the_wavefront_kernels(da):
    """65 .. 300 residues: one wavefront per pair (k_nw_long), float64 on the host boundary (lengths beyond the uint16 code)"""
    from dynaalign_amd import device, _capi
    rng = np.random.RandomState(9)
    x, y = two_sets(rng, 9, 11, AA24, 60, 300)
    want, _, _, _ = nw_expected(x, y, "BLOSUM62", 10, 4)
    assert same(da.similarityNW_cross(x, y), want)
    assert same(host_cross_nw(x, y, "BLOSUM62", 10, 4, 1), want.T)
    _, _, dxy = device_sets(x, y)
    device.nw_encode(dxy)
    assert same(device.nw_rect(dxy, "BLOSUM62", 10, 4, 9, 20, 0, 9, _capi.DA_OUT_F64).cpu().numpy(), want.T)


@pytest.mark.parametrize("m,n", [(3, 700), (700, 3), (4, 650), (650, 4), (1, 300), (130, 257)])
def test_host_calls_in_several_row_blocks(da, m, n):
    """results far taller or wider than a row block (DYNAALIGN_BLOCK_BYTES holds 128 rows: the smallest block), both layouts, odd and even
    column counts: every block starts on a multiple of 128 rows and lands where it belongs"""
    rng = np.random.RandomState(m * 1000 + n)
    x, y = two_sets(rng, m, n, AA24)
    seeds = O.seeds(SEED, 50)
    want = O.similarity_mh(x + y, 4, 50, seeds)[1][:m, m:]
    want_nw, _, _, _ = nw_expected(x, y, "BLOSUM62", 10, 4)
    for widen in (False, True):
        env = {"DYNAALIGN_BLOCK_BYTES": 1024}
        if not widen:
            env["DYNAALIGN_NO_HOST_WIDEN"] = 1
        with switches(**env):
            assert same(host_cross_mh(x, y, 4, 50, seeds, 0), want) and same(host_cross_mh(x, y, 4, 50, seeds, 1), want.T), (m, n, widen)
            assert same(host_cross_nw(x, y, "BLOSUM62", 10, 4, 0), want_nw) and same(host_cross_nw(x, y, "BLOSUM62", 10, 4, 1), want_nw.T), (m, n, widen)
            # the square calls share the row-block loop
            assert same(da.similarityMH(x + y, 4, 50, seed=SEED), O.similarity_mh(x + y, 4, 50, seeds)[1])


# ---- medium: every route on the headline generator ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def h3n2_two_sets(da):
    from dynaalign_amd import synth
    x = synth.to_strings(*synth.h3n2_like(3000, seed_samples=13))
    y = synth.to_strings(*synth.h3n2_like(5000, seed_samples=17))
    seeds = O.seeds(SEED, 500)
    cnt = O.mh_counts(O.signatures(x + y, 4, 500, seeds), 0, 3000)[:, 3000:]
    return x, y, seeds, cnt


def test_medium_h3n2_every_route(da, h3n2_two_sets):
    from dynaalign_amd import device, session
    x, y, seeds, cnt = h3n2_two_sets
    m, n = len(x), len(y)
    want = cnt.astype(np.float64) / 500.0                            # the reference's divide
    # what makes this input a test of the shared dictionary: many strings on both sides, agreeing only through their codes
    assert (len(set(x)), len(set(y)), len(set(x) & set(y))) == (2202, 3313, 738)
    assert int((cnt == 500).sum()) == 4366 and len(np.unique(cnt)) == 467
    dx, dy, _ = device_sets(x, y)
    with switches(DYNAALIGN_MH_NO_DEDUP=1):
        direct = device.similarity_mh_cross(dx, dy, 4, 500, seeds)
        torch.cuda.synchronize()
        route = device.mh_cross_last_route()
    assert not route["dedup"] and route["plane_bits"] == 12, route
    assert same(direct.cpu().numpy(), want)
    with switches(DYNAALIGN_MH_DEDUP_MAX_PCT=100):
        dup = device.similarity_mh_cross(dx, dy, 4, 500, seeds)
        torch.cuda.synchronize()
        route = device.mh_cross_last_route()
    assert route["dedup"] and (route["unique_x"], route["unique_y"]) == (2202, 3313), route
    assert same(dup.cpu().numpy(), want)
    # the built-in rule on this input (sqrt(2202 * 3313 / (3000 * 5000)) = 0.697 > 0.68): the direct route, with the plans' counts reported
    out = device.similarity_mh_cross(dx, dy, 4, 500, seeds)
    torch.cuda.synchronize()
    route = device.mh_cross_last_route()
    assert not route["dedup"] and (route["unique_x"], route["unique_y"]) == (2202, 3313)
    assert same(out.cpu().numpy(), want)
    # the host boundary and the session
    assert same(da.similarityMH_cross(x, y, 4, 500, seed=SEED), want)
    assert same(host_cross_mh(x, y, 4, 500, seeds, 1), want.T)
    s = session.MinHashSession(y, 4, 500, seed=SEED, reserve=False)
    assert same(s.cross(x), want)
    assert same(s.cross(x), da.similarityMH_cross(x, y, 4, 500, seed=SEED))
    idx = np.arange(n - 1, -1, -3)
    assert same(s.cross(x[:700], idx), want[:700][:, idx])


def test_medium_uniform_takes_the_direct_route_by_itself(da):
    from dynaalign_amd import device, synth
    x = synth.to_strings(*synth.uniform_peptides(1000, seed=7))
    y = synth.to_strings(*synth.uniform_peptides(1500, seed=8))
    seeds = O.seeds(SEED, 500)
    cnt = O.mh_counts(O.signatures(x + y, 4, 500, seeds), 0, 1000)[:, 1000:]
    assert int((cnt != 0).sum()) == 2599 and not (set(x) & set(y))
    dx, dy, _ = device_sets(x, y)
    out = device.similarity_mh_cross(dx, dy, 4, 500, seeds)
    torch.cuda.synchronize()
    route = device.mh_cross_last_route()
    assert not route["dedup"] and (route["unique_x"], route["unique_y"]) == (1000, 1500), route
    assert same(out.cpu().numpy(), cnt.astype(np.float64) / 500.0)


@pytest.mark.parametrize("which", ["h3n2", "uniform"])
def test_medium_nw_order_matters(da, which):
    """calc(x_i, y_j) != calc(y_j, x_i) for some pairs of these sets: an implementation that swaps the operands cannot pass"""
    from dynaalign_amd import device, synth, _capi
    if which == "h3n2":
        x = synth.to_strings(*synth.h3n2_like(3000, seed_samples=13))[:400]
        y = synth.to_strings(*synth.h3n2_like(5000, seed_samples=17))[:600]
        asym_want, gapped_want = 70, 36960
    else:
        x = synth.to_strings(*synth.uniform_peptides(1000, seed=7))[:400]
        y = synth.to_strings(*synth.uniform_peptides(1500, seed=8))[:600]
        asym_want, gapped_want = 96, 37080
    m, n = len(x), len(y)
    want, want_code, nm, ln = nw_expected(x, y, "BLOSUM62", 10, 4)
    rc, nm_s, ln_s, _, _ = O.nw_rows(y + x, 0, n)                    # the swapped evaluation: calc(y_j, x_i)
    assert rc == 0
    swapped = (nm_s[:, n:].T != nm) | (ln_s[:, n:].T != ln)
    assert int(swapped.sum()) >= 1
    assert (int(swapped.sum()), int((ln > 20).sum())) == (asym_want, gapped_want)
    assert same(da.similarityNW_cross(x, y), want)
    assert same(host_cross_nw(x, y, "BLOSUM62", 10, 4, 1), want.T)
    _, _, dxy = device_sets(x, y)
    device.nw_encode(dxy)
    c = device.nw_rect(dxy, "BLOSUM62", 10, 4, 0, m, m, m + n, _capi.DA_OUT_COMPACT).cpu().numpy().view(np.uint16)
    assert np.array_equal(c >> 8, nm) and np.array_equal(c & 255, ln)
    tc = device.nw_rect(dxy, "BLOSUM62", 10, 4, m, m + n, 0, m, _capi.DA_OUT_COMPACT).cpu().numpy().view(np.uint16)
    assert np.array_equal(tc, c.T)
    f = device.nw_rect(dxy, "BLOSUM62", 10, 4, 0, m, m, m + n, _capi.DA_OUT_F64).cpu().numpy()
    assert same(f, nm.astype(np.float64) / ln.astype(np.float64)) and same(f, want)
