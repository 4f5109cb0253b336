"""The zoned id order of the MinHash duplicate plan, host side (da_common.hpp zoned_rank through da_debug_zoned_ids; no GPU): the single-copy
strings of zone z are numbered M + rank of (q, z), q their rank inside the zone, among all pairs in lexicographic order.  The map must be a
bijection onto [M, M + sum h) and increasing in (q, z) for any zone sizes h."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def zoned_ids(built):
    from dynaalign_amd import _capi
    fn = _capi.load().da_debug_zoned_ids
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p]
    fn.restype = ctypes.c_int

    def call(h, M):
        h = np.ascontiguousarray(h, np.int32)
        out = np.full(int(h.sum()) + 1, -7, np.int64)
        assert fn(h.ctypes.data, len(h), M, out.ctypes.data) == 0
        assert out[-1] == -7                                             # nothing written past sum h
        return out[:-1]
    return call


def cases():
    rng = np.random.RandomState(18)
    out = [("all_zero", [0] * 8, 5), ("one_zone_holds_everything", [0, 0, 0, 977, 0, 0, 0, 0], 3), ("last_zone_only", [0] * 7 + [64], 0),
           ("zones_1", [1234], 17), ("zones_1_empty", [0], 4), ("equal", [125] * 8, 3064), ("second_half_empty", [310, 290, 305, 295, 0, 0, 0, 0], 100),
           ("very_unequal", [1, 4000, 0, 2, 999, 1, 0, 63], 9), ("three_zones", [5, 0, 9], 2), ("ones", [1] * 8, 0)]
    for t in range(12):
        zones = int(rng.randint(1, 9))
        h = rng.randint(0, [3, 40, 3000][t % 3], zones)
        h[rng.rand(zones) < 0.25] = 0
        out.append(("random%d" % t, h.tolist(), int(rng.randint(0, 5000))))
    return out


@pytest.mark.parametrize("name,h,M", cases(), ids=[c[0] for c in cases()])
def test_zoned_ids_are_a_bijection_in_lexicographic_order(zoned_ids, name, h, M):
    h = np.asarray(h, np.int64)
    ids = zoned_ids(h, M)
    total = int(h.sum())
    assert len(ids) == total
    assert np.array_equal(np.sort(ids), M + np.arange(total))            # a bijection onto [M, M + sum h)
    z = np.repeat(np.arange(len(h)), h)                                  # the entry's order: zone after zone, q ascending
    q = np.concatenate([np.arange(x) for x in h]) if total else np.zeros(0, np.int64)
    by_qz = np.lexsort((z, q))                                           # (q, z) lexicographic: q first, then z
    assert np.array_equal(ids[by_qz], M + np.arange(total))              # increasing in that order (with the bijection: exactly the rank)


def test_zoned_ids_rejects_bad_arguments(zoned_ids, built):
    from dynaalign_amd import _capi
    fn = _capi.load().da_debug_zoned_ids
    h = np.ones(9, np.int32)
    out = np.zeros(16, np.int64)
    assert fn(h.ctypes.data, 9, 0, out.ctypes.data) != 0                 # more zones than the expansion has
    assert fn(h.ctypes.data, 0, 0, out.ctypes.data) != 0
    assert fn(None, 8, 0, out.ctypes.data) != 0
