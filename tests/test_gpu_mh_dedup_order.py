"""GPU tests of the zoned id order of the MinHash duplicate plan (nw_kernels.hip k_dd_assign, DedupOrder::zoned): multi-copy strings first by
first occurrence, then the single-copy strings dealt round-robin over the eight row zones of the row expansion.  The numbering is read back
through da_debug_mh_dedup_ids; the n x n matrix of the `rows` and `rowspipe` forms must be bit-identical with the zoned order, with ids by first
occurrence (DYNAALIGN_MH_DEDUP_ORDER=first) and on the direct route."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
from test_gpu_expand_zones import duplicated, env, pool_of, run, same

pytestmark = pytest.mark.gpu

MULTI_FIRST, FIRST, ZONED = 0, 1, 2
DEFAULT_ORDER = ZONED                                                   # what the row forms take when DYNAALIGN_MH_DEDUP_ORDER is not set


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    from dynaalign_amd import _capi
    assert _capi.load().da_device_count() > 0
    return dynaalign_amd


# ---- the numbering -------------------------------------------------------------------------------------------------------------------------------

def dedup_ids(seqs, order, zones):
    """da_debug_mh_dedup_ids: (uidx[n], U, M)"""
    import torch
    from dynaalign_amd import _capi
    fn = _capi.load().da_debug_mh_dedup_ids
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_void_p, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    res, off = O.pack(seqs)
    res, off = np.asarray(res, np.uint8), np.asarray(off, np.int64)
    n = len(seqs)
    d_res, d_off = torch.from_numpy(res.copy()).cuda(), torch.from_numpy(off.copy()).cuda()
    d_uidx = torch.full((n + 4,), -9, dtype=torch.int32, device="cuda")
    U, M = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert fn(d_res.data_ptr(), d_off.data_ptr(), n, int(off[-1]), order, zones, d_uidx.data_ptr(), ctypes.addressof(U), ctypes.addressof(M), None) == 0
    torch.cuda.synchronize()
    u = d_uidx.cpu().numpy().astype(np.int64)
    assert (u[n:] == -9).all()
    return u[:n], U.value, M.value


def check_ids(seqs, uidx, U, M, order, zones):
    n = len(seqs)
    first, count = {}, {}
    for i, s in enumerate(seqs):
        first.setdefault(s, i)
        count[s] = count.get(s, 0) + 1
    assert U == len(first) and M == sum(1 for c in count.values() if c > 1)
    # equal ids exactly for equal strings, and the ids are a permutation of [0, U)
    rep = np.array([first[s] for s in seqs])
    assert np.array_equal(uidx, uidx[rep])
    reps = np.flatnonzero(rep == np.arange(n))                           # first occurrences, ascending
    assert np.array_equal(np.sort(uidx[reps]), np.arange(U))
    multi = np.array([count[seqs[i]] > 1 for i in reps], bool)
    if order == FIRST:
        assert np.array_equal(uidx[reps], np.arange(U))
        return
    # ids < M: exactly the multi-copy strings, in order of first occurrence
    assert np.array_equal(uidx[reps[multi]], np.arange(M))
    singles = reps[~multi]
    if order == MULTI_FIRST:
        assert np.array_equal(uidx[singles], M + np.arange(U - M))
        return
    # zoned: within a zone the singles keep their row order, and in every prefix of the single ids the zones not yet exhausted have
    # received the same number of ids, to within one
    Z = -(-n // zones)
    home = singles // Z
    h = np.bincount(home, minlength=zones)
    for z in range(zones):
        assert (np.diff(uidx[singles[home == z]]) > 0).all()
    by_id = home[np.argsort(uidx[singles])]                              # home zone of the ids M, M + 1, ...
    given = np.cumsum(by_id[:, None] == np.arange(zones)[None, :], axis=0)
    for p in range(len(by_id)):
        live = given[p] < h
        if live.any():
            assert given[p][live].max() - given[p][live].min() <= 1, (p, given[p], h)
    return h


def id_cases():
    out = {}
    rng = np.random.RandomState(3301)
    out["pool"] = duplicated(rng, 2300, extra=1300)                      # n = 3600: multi- and single-copy strings everywhere
    rng = np.random.RandomState(3302)
    out["pool_n_not_multiple_of_8"] = duplicated(rng, 2200, extra=1411)  # n = 3611
    rng = np.random.RandomState(3303)
    pool = pool_of(rng, 1600)
    s = pool + pool
    rng.shuffle(s)
    out["no_singles"] = s                                                # every string twice
    rng = np.random.RandomState(3304)
    pool = pool_of(rng, 3000)
    head = pool[:400] + [pool[q] for q in rng.randint(0, 400, 500)]     # rows 0 ... 899 (zones 0 and 1 of 8 x 438): strings with copies;
    rng.shuffle(head)
    out["multi_only_in_zones_0_1"] = head + pool[400:]                   # rows 900 ...: 2600 single-copy strings, n = 3500
    rng = np.random.RandomState(3305)
    pool = pool_of(rng, 1750)
    out["second_half_copies_first"] = pool + pool                        # n = 3500, no singles; every first occurrence in zones 0 - 3
    rng = np.random.RandomState(3306)
    pool = pool_of(rng, 1802)                                            # n = 3604, Z = 451: rows 0 ... 900 and their copies in rows 1802 ... are
    out["second_half_copies_first_quarter"] = pool + pool[:901] + pool[:901]   # multi-copy; the singles are rows 901 ... 1801: h = 0 but in zones 1 - 3
    out["n9"] = [pool[q] for q in (0, 1, 0, 2, 3, 4, 2, 5, 6)]           # Z = 2: zones 5 - 7 lie past the input
    return out


@pytest.mark.parametrize("zones", [8, 1])
@pytest.mark.parametrize("case", sorted(id_cases()))
def test_zoned_ids(da, case, zones):
    seqs = id_cases()[case]
    n = len(seqs)
    uidx, U, M = dedup_ids(seqs, ZONED, zones)
    h = check_ids(seqs, uidx, U, M, ZONED, zones)
    if case.startswith("pool"):
        assert 3000 <= n <= 4000 and M > 0 and (h > 0).all()
    if case == "pool_n_not_multiple_of_8":
        assert n % 8 != 0
    if case in ("no_singles", "second_half_copies_first"):
        assert M == U and h.sum() == 0
    if case == "multi_only_in_zones_0_1" and zones == 8:
        assert M <= 400 and h[2:].sum() >= 2600 and (h[3:7] == 438).all() and h[7] == 434   # zones 3 - 7: single-copy strings only
    if case == "second_half_copies_first_quarter" and zones == 8:
        assert M == 901 and h[0] == 0 and (h[4:] == 0).all() and h[1:4].sum() == 901 and (h[1:4] > 0).all()


def test_other_orders_and_the_call_default(da):
    """the two orders that were there before, and zones = 0 (what a call uses: eight zones unless DYNAALIGN_MH_EXPAND_ZONES=1)"""
    seqs = id_cases()["pool"]
    for order in (MULTI_FIRST, FIRST):
        uidx, U, M = dedup_ids(seqs, order, 1)
        check_ids(seqs, uidx, U, M, order, 1)
    u8, U, M = dedup_ids(seqs, ZONED, 8)
    u1, _, _ = dedup_ids(seqs, ZONED, 1)
    assert not np.array_equal(u8, u1)
    assert np.array_equal(dedup_ids(seqs, ZONED, 0)[0], u8)
    with env(DYNAALIGN_MH_EXPAND_ZONES=1):
        assert np.array_equal(dedup_ids(seqs, ZONED, 0)[0], u1)
    # one zone: multi-copy first, then the singles by first occurrence
    assert np.array_equal(u1, dedup_ids(seqs, MULTI_FIRST, 1)[0])


# ---- the whole matrix ----------------------------------------------------------------------------------------------------------------------------

DEDUP = dict(DYNAALIGN_MH_DEDUP_MIN_N=1, DYNAALIGN_PLANE_BITS=12)
FORMS = {"rows": "rows", "rowspipe": "rows, pipelined"}
ORDER_NAMES = {FIRST: "first", ZONED: "zoned"}


def last_order():
    from dynaalign_amd import _capi
    fn = _capi.load().da_debug_mh_last_dedup_order
    fn.argtypes, fn.restype = [ctypes.c_void_p], ctypes.c_int
    o = ctypes.c_int(-5)
    assert fn(ctypes.addressof(o)) == 0
    return o.value


def matrix_cases():
    return {
        "u1537_h500": (1537, None, 500, {}),
        "u1537_h600": (1537, None, 600, {}),
        "u3100_h500_chunks": (3100, None, 500, dict(DYNAALIGN_MH_PIPE_HEAD=1, DYNAALIGN_MH_PIPE_STEP=1)),
        "u1300_h600_odd_n": (1300, 1301, 600, {}),
        "u1537_h500_one_zone": (1537, None, 500, dict(DYNAALIGN_MH_EXPAND_ZONES=1)),
    }


@pytest.mark.parametrize("case", sorted(matrix_cases()))
def test_row_forms_zoned_against_first_and_direct(da, case):
    U, extra, n_hash, more = matrix_cases()[case]
    seqs = duplicated(np.random.RandomState(U), U, extra=extra)
    n = len(seqs)
    assert len(set(seqs)) == U and (n % 2 == 1) == ("odd_n" in case)
    direct, droute = run(seqs, 4, n_hash, DYNAALIGN_MH_NO_DEDUP=1)
    assert not droute["dedup"] and last_order() == -1
    out = None
    if n % 2:                                                           # the row forms want an even leading dimension: an odd n in a padded output
        import torch
        out = torch.full((n, n + 5), -1.0, dtype=torch.float64, device="cuda")[:, :n]
    for form, name in FORMS.items():
        for order in (FIRST, ZONED):
            got, route = run(seqs, 4, n_hash, out=out, DYNAALIGN_MH_EXPAND=form, DYNAALIGN_MH_DEDUP_ORDER=ORDER_NAMES[order], **DEDUP, **more)
            assert route["dedup"] and route["unique"] == U and route["expansion"] == name, route
            assert last_order() == order
            assert bool(n_hash <= 511) == packed_table()
            if "chunks" in case and form == "rowspipe":
                assert route["chunks"] >= 4, route
            assert same(got, direct), (case, form, order)
        del got


def packed_table():
    from dynaalign_amd import _capi
    fn = _capi.load().da_debug_mh_last_table_packed
    fn.argtypes, fn.restype = [ctypes.c_void_p], ctypes.c_int
    p = ctypes.c_int(-1)
    assert fn(ctypes.addressof(p)) == 0
    return bool(p.value)


def test_default_order_of_the_forms(da):
    """without the switch: the row forms take DEFAULT_ORDER, the tile forms ids by first occurrence (their schedule relies on it) whatever the switch"""
    seqs = duplicated(np.random.RandomState(1537), 1537)
    direct, _ = run(seqs, 4, 500, DYNAALIGN_MH_NO_DEDUP=1)
    got, route = run(seqs, 4, 500, DYNAALIGN_MH_EXPAND="rowspipe", **DEDUP)
    assert route["expansion"] == "rows, pipelined" and last_order() == DEFAULT_ORDER and same(got, direct)
    for form in ("tiles", "pipe"):
        got, route = run(seqs, 4, 500, DYNAALIGN_MH_EXPAND=form, DYNAALIGN_MH_DEDUP_ORDER="zoned", **DEDUP)
        assert route["dedup"] and route["expansion"].startswith("tiles") and last_order() == FIRST and same(got, direct)
