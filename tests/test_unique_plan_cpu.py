"""CPU tests of the duplicate plan's model (tests/unique_plan_model.py; no GPU): its port of the table hash equals the library's (da_common.hpp
dd_hash through da_debug_dd_hash), its own invariants hold on every input the GPU tests feed the device, and `colliding` delivers the start slots
the probe-chain test relies on."""
import ctypes

import numpy as np
import pytest

import unique_plan_model as P


@pytest.fixture(scope="module")
def lib_hash(built):
    from dynaalign_amd import _capi
    fn = _capi.load().da_debug_dd_hash
    fn.argtypes, fn.restype = [ctypes.c_char_p, ctypes.c_int32, ctypes.c_void_p], ctypes.c_int

    def h(b):
        out = ctypes.c_uint32(0)
        assert fn(b, len(b), ctypes.addressof(out)) == 0
        return out.value
    return h


def test_hash_port_equals_the_library(lib_hash):
    rng = np.random.RandomState(4401)
    strings = [b"", b"\x00", b"\xff", b"\x00\x00", b"\xff\xff", b"\x00" * 70, b"\xff" * 70, b"\x80" * 33]
    for L in range(71):                                                            # every length 0 ... 70, forty strings each
        for _ in range(40):
            alpha = [(0, 256), (0, 2), (254, 256)][rng.randint(3)]                 # all bytes / 0x00 and 0x01 / 0xFE and 0xFF
            strings.append(rng.randint(alpha[0], alpha[1], L).astype(np.uint8).tobytes())
    strings += [s + b"\xff" for s in strings[8:400]] + [b"\x00" + s for s in strings[8:400]]
    assert len(strings) > 3000 and {len(s) for s in strings} >= set(range(71))
    assert any(0x00 in s for s in strings) and any(0xFF in s for s in strings)
    for s in strings:
        assert P.dd_hash(s) == lib_hash(s), s
    # the length enters the hash: strings of zero bytes of different lengths differ, and so does the cut of "ABC"
    assert len({P.dd_hash(b"\x00" * k) for k in range(8)}) == 8
    # ... and the bulk form is the same function
    a = rng.randint(0, 256, (500, 13)).astype(np.uint8)
    assert P.dd_hash_rows(a).tolist() == [P.dd_hash(r.tobytes()) for r in a]
    assert P.dd_hash_rows(np.zeros((3, 0), np.uint8)).tolist() == [P.dd_hash(b"")] * 3


def test_null_arguments_are_refused(built):
    from dynaalign_amd import _capi
    fn = _capi.load().da_debug_dd_hash
    fn.argtypes, fn.restype = [ctypes.c_char_p, ctypes.c_int32, ctypes.c_void_p], ctypes.c_int
    out = ctypes.c_uint32(0)
    assert fn(None, 0, ctypes.addressof(out)) == 0 and out.value == P.dd_hash(b"")
    assert fn(None, 3, ctypes.addressof(out)) != 0
    assert fn(b"abc", -1, ctypes.addressof(out)) != 0
    assert fn(b"abc", 3, None) != 0


def test_table_size():
    assert [P.table_size(n) for n in (1, 512, 513, 600, 1024, 1025, 8192, 20000)] == [1024, 1024, 2048, 2048, 2048, 4096, 16384, 65536]
    assert P.table_size(P.CHAIN_N) == P.CHAIN_TS


@pytest.mark.parametrize("case", sorted(P.all_plan_inputs()))
def test_model_invariants(case):
    seqs = P.all_plan_inputs()[case]
    n = len(seqs)
    m = P.plan_model(seqs)
    U, M = m["U"], m["M"]
    assert U == len(set(seqs)) and 0 <= M <= U
    assert np.array_equal(m["uidx"][m["ufirst"]], np.arange(U))                   # uidx[ufirst] is the identity
    assert np.array_equal(m["uidx"][m["ulast"]], np.arange(U))
    assert (m["ufirst"] <= m["ulast"]).all() and m["ufirst"].min() == 0 and m["ulast"].max() == n - 1
    assert np.array_equal(np.unique(m["uidx"]), np.arange(U))                     # the ids are a permutation of [0, U)
    lo, hi = np.full(U, n), np.full(U, -1)                                         # first / last row of every id, the numpy way
    np.minimum.at(lo, m["uidx"], np.arange(n))
    np.maximum.at(hi, m["uidx"], np.arange(n))
    assert np.array_equal(lo, m["ufirst"]) and np.array_equal(hi, m["ulast"])
    assert all(seqs[i] == seqs[m["ufirst"][m["uidx"][i]]] for i in range(n))        # equal ids only for equal strings
    # multi-copy strings first, each group by first occurrence
    copies = np.bincount(m["uidx"], minlength=U)
    assert (copies[:M] > 1).all() and (copies[M:] == 1).all()
    assert (np.diff(m["ufirst"][:M]) > 0).all() and (np.diff(m["ufirst"][M:]) > 0).all()
    assert (m["ufirst"][M:] == m["ulast"][M:]).all() and (m["ufirst"][:M] < m["ulast"][:M]).all()
    # the strings back to back in id order
    off = m["uoffsets"]
    assert off[0] == 0 and off[-1] == len(m["ubytes"]) and (np.diff(off) >= 0).all()
    for i in range(0, n, max(1, n // 200)):
        u = m["uidx"][i]
        assert m["ubytes"][off[u]:off[u + 1]] == seqs[i]
    # the block arrays bound their 64 ids
    for b in range(len(m["minfirst"])):
        assert m["minfirst"][b] <= m["ufirst"][b * 64:(b + 1) * 64].min() and m["maxlast"][b] >= m["ulast"][b * 64:(b + 1) * 64].max()
        assert m["minfirst"][b] in m["ufirst"][b * 64:(b + 1) * 64] and m["maxlast"][b] in m["ulast"][b * 64:(b + 1) * 64]
    assert len(m["minfirst"]) == len(m["maxlast"]) == -(-U // 64)


def test_the_cases_are_what_their_names_say():
    for name, (seqs, n, U) in P.size_cases().items():
        assert len(seqs) == n and len(set(seqs)) == U and all(len(s) <= 70 for s in seqs), name
    assert {n for _, n, _ in P.size_cases().values()} >= {1, 2, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 9217, 20000}
    assert {U for _, n, U in P.size_cases().values() if n == 20000} == {8191, 8192, 8193, 12353}
    d = {k: P.plan_model(v) for k, v in P.degenerate_cases().items()}
    assert (d["all_equal_8192"]["U"], d["all_equal_8192"]["M"]) == (1, 1)
    assert (d["all_distinct_8192"]["U"], d["all_distinct_8192"]["M"]) == (8192, 0)
    assert d["every_string_twice"]["U"] == d["every_string_twice"]["M"] == 4500
    assert (d["five_empty"]["U"], len(d["five_empty"]["ubytes"])) == (1, 0)
    c = P.content_cases()
    assert c["abc_cut_two_ways"][:4] == [b"AB", b"C", b"A", b"BC"] and c["empty_among_others"].count(b"") > 50
    assert P.plan_model(c["abc_cut_two_ways"])["U"] == 6
    for seqs in P.order_cases().values():
        assert all(len(s) <= 70 for s in seqs) and sum(map(len, seqs)) > 0


def test_colliding_delivers_its_slots():
    rng = np.random.RandomState(4402)
    for slots, count, length in (([2045, 2046, 2047], 48, 9), ([0, 1], 24, 10), ([1234], 200, 11), ([5], 3, 1 + 2)):
        got = P.colliding(rng, 2048, slots, count, length)
        assert len(got) == count == len(set(got)) and all(len(s) == length for s in got)
        assert all(P.dd_hash(s) & 2047 in slots for s in got)
    seqs, groups = P.probe_chain_case()
    assert len(seqs) == P.CHAIN_N == 600 and P.table_size(len(seqs)) == 2048
    for name, (strings, slots) in groups.items():
        assert all(P.dd_hash(s) & 2047 in slots for s in strings) and all(s in seqs for s in strings), name
    assert len(set(seqs)) == 48 + 24 + 200 + 300
