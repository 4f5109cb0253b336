"""Plain Python / numpy model of the duplicate plan (nw_kernels.hip "duplicate sequences", da_dev_unique_plan) and the inputs its tests
share.  TEST INFRASTRUCTURE: test_unique_plan_cpu.py checks the model against itself and its hash against the library's (da_debug_dd_hash);
test_gpu_unique_plan.py compares every field the device writes with it.

The plan numbers the distinct strings of an input multi-copy first: strings that occur more than once get the ids 0 ... M - 1 in order of first
occurrence, the others M ... U - 1 in order of occurrence.  Strings are bytes objects here (the MinHash route plans on raw bytes)."""
import functools

import numpy as np

BLOCK = 64                                     # ids per entry of minfirst / maxlast (one tile row of the ordered NW sweep)


def plan_model(seqs):
    """-> dict(U, M, uidx[n], ufirst[U], ulast[U], uoffsets[U + 1], ubytes (bytes), minfirst[ceil(U / 64)], maxlast[ceil(U / 64)])"""
    first, last, count = {}, {}, {}
    for i, s in enumerate(seqs):
        first.setdefault(s, i)                 # (dicts keep insertion order: `first` lists the strings by first occurrence)
        last[s] = i
        count[s] = count.get(s, 0) + 1
    order = [s for s in first if count[s] > 1]
    M = len(order)
    order += [s for s in first if count[s] == 1]
    U = len(order)
    uid = {s: u for u, s in enumerate(order)}
    ufirst = np.array([first[s] for s in order], np.int64)
    ulast = np.array([last[s] for s in order], np.int64)
    uoffsets = np.zeros(U + 1, np.int64)
    uoffsets[1:] = np.cumsum([len(s) for s in order])
    nb = -(-U // BLOCK)
    return {"U": U, "M": M, "uidx": np.array([uid[s] for s in seqs], np.int64), "ufirst": ufirst, "ulast": ulast, "uoffsets": uoffsets,
            "ubytes": b"".join(order),
            "minfirst": np.array([ufirst[b * BLOCK:(b + 1) * BLOCK].min() for b in range(nb)], np.int64),
            "maxlast": np.array([ulast[b * BLOCK:(b + 1) * BLOCK].max() for b in range(nb)], np.int64)}


# ---- the hash that picks a string's start slot (da_common.hpp dd_hash) ---------------------------------------------------------------------------

_M32 = 0xFFFFFFFF


def dd_hash(b):
    h = 0x9747B28C ^ len(b)
    for c in b:
        h ^= c
        h = (h * 0x01000193) & _M32
        h ^= h >> 15
    h ^= h >> 13
    h = (h * 0x5BD1E995) & _M32
    h ^= h >> 15
    return h


def dd_hash_rows(a):
    """dd_hash of every row of a uint8 array [count][length] (strings of one length), as uint32[count]"""
    a = np.asarray(a, np.uint8)
    h = np.full(a.shape[0], 0x9747B28C ^ a.shape[1], np.uint32)
    for q in range(a.shape[1]):
        h ^= a[:, q]
        h *= np.uint32(0x01000193)
        h ^= h >> np.uint32(15)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0x5BD1E995)
    h ^= h >> np.uint32(15)
    return h


def table_size(n):
    """slots of the plan's table (nw_dedup_layout): 1024 doubled until it is at least 2 n"""
    ts = 1024
    while ts < 2 * n:
        ts *= 2
    return ts


def colliding(rng, ts, slots, count, length):
    """`count` distinct strings of `length` bytes whose start slot dd_hash & (ts - 1) lies in `slots`, found among random strings hashed in bulk"""
    slots = np.asarray(sorted(slots), np.uint32)
    found, seen = [], set()
    while len(found) < count:
        a = rng.randint(0, 256, (1 << 17, length)).astype(np.uint8)
        hit = np.flatnonzero(np.isin(dd_hash_rows(a) & np.uint32(ts - 1), slots))
        for r in hit:
            s = a[r].tobytes()
            if s not in seen and len(found) < count:
                seen.add(s)
                found.append(s)
    return found


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------------

_HARD = np.array([0x00, 0x80, 0xFF, 0x41, 0x42, 0x43], np.uint8)
_FIXED = [b"", b"AB", b"C", b"A", b"BC", b"ABC", b"\x00", b"\x00\x00", b"\x80", b"\xff", b"\xff\xff", b"\x00\xff", b"\xff\x00"]


def hostile_pool(rng, U, max_len=70):
    """exactly U distinct strings of 0 ... max_len bytes, in random order: the empty string, the pieces of "ABC", raw bytes 0x00 / 0x80 / 0xFF
    alone and in runs, and families of random strings -- over all byte values or over six of them -- with proper prefixes of each other and
    strings that differ in the last byte only"""
    pool, seen = [], set()

    def add(s):
        if s not in seen and len(pool) < U:
            seen.add(s)
            pool.append(s)

    for s in _FIXED:
        add(s)
    while len(pool) < U:
        L = int(rng.randint(1, max_len + 1))
        base = (_HARD[rng.randint(0, len(_HARD), L)] if rng.rand() < 0.3 else rng.randint(0, 256, L).astype(np.uint8)).tobytes()
        add(base)
        add(base[:int(rng.randint(0, L + 1))])                                   # a prefix
        add(base[:-1])                                                           # the longest proper prefix
        add(base[:-1] + bytes([(base[-1] + 1 + int(rng.randint(0, 255))) % 256]))   # the last byte differs
        add(base[:-1] + bytes([base[-1] ^ 0x80]))
    order = rng.permutation(U)
    return [pool[q] for q in order]


def with_unique(rng, n, U, max_copies=None):
    """n rows over exactly U distinct hostile strings in random row order; max_copies bounds the copies of one string (None: free)"""
    assert 1 <= U <= n
    pool = hostile_pool(rng, U)
    if max_copies is None:
        extra = [pool[q] for q in rng.randint(0, max(1, U // 3), n - U)]         # copies of the first third: many strings stay single
    else:
        assert U * max_copies >= n
        extra = [pool[q] for q in rng.permutation(np.repeat(np.arange(U), max_copies - 1))[:n - U]]
    seqs = pool + extra
    return [seqs[q] for q in rng.permutation(n)]


@functools.lru_cache(None)
def size_cases():
    """name -> (seqs, n, U): one input per size at which the plan changes its path (the one-workgroup scans step by 1024, from 8192 elements
    on three launches scan: over n for the flags, over U for the offsets)"""
    out = {}
    for n in (1, 2, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 9217):
        U = max(1, (2 * n) // 3)
        out["n%d" % n] = (with_unique(np.random.RandomState(7000 + n), n, U), n, U)
    out["n2_distinct"] = ([b"\x00", b""], 2, 2)
    for U in (8191, 8192, 8193, 12353):
        out["n20000_u%d" % U] = (with_unique(np.random.RandomState(9000 + U), 20000, U), 20000, U)
    return out


@functools.lru_cache(None)
def degenerate_cases():
    out = {}
    rng = np.random.RandomState(7101)
    out["all_equal_8192"] = [b"MKTIIALSYIFCLVFA"] * 8192
    out["all_distinct_8192"] = with_unique(rng, 8192, 8192)
    pool = hostile_pool(rng, 4500)
    out["every_string_twice"] = [(pool + pool)[q] for q in rng.permutation(9000)]
    out["five_empty"] = [b""] * 5
    return out


@functools.lru_cache(None)
def content_cases():
    out = {}
    out["abc_cut_two_ways"] = [b"AB", b"C", b"A", b"BC", b"AB", b"C", b"ABC", b"A", b"", b"BC", b"", b"ABC", b""]
    out["raw_bytes"] = [b"\x00", b"\x00\x00", b"", b"\xff", b"\x80", b"\x00", b"\xff\xff", b"\x80\x00", b"\x00\x80", b"\xff", b"", b"\x00\x00\x00",
                        b"\x00\x00", b"\x7f", b"\x80"]
    fam = [b"ACDEFGHIKLMNPQRSTVWY"[:k] for k in range(21)]                           # every prefix of one string, the empty one included
    fam += [b"ACDEFGHIKLMNPQRSTVW" + bytes([c]) for c in (0x00, 0x58, 0x59 ^ 0x80, 0xFF)]   # ... and strings that differ from it in the last byte
    rng = np.random.RandomState(7102)
    out["prefixes_and_last_byte"] = [fam[q] for q in rng.randint(0, len(fam), 200)] + fam[::-1]
    out["empty_among_others"] = [(b"" if q % 7 in (0, 3) else s) for q, s in enumerate(with_unique(rng, 300, 200))]
    return out


CHAIN_N, CHAIN_TS = 600, 2048


@functools.lru_cache(None)
def probe_chain_case():
    """-> (seqs, groups): n = 600 rows, a table of 2048 slots.  groups["wrap"]: 48 distinct strings that start in the last three slots (they cannot
    fit there: the chain wraps to slot 0), 1 - 3 copies each; groups["displaced"]: 24 that start in slots 0 and 1; groups["chain"]: 200 that share
    one start slot; the rest random strings; random row order"""
    rng = np.random.RandomState(7103)
    ts = CHAIN_TS
    wrap = colliding(rng, ts, [ts - 3, ts - 2, ts - 1], 48, 9)
    displaced = colliding(rng, ts, [0, 1], 24, 10)
    chain = colliding(rng, ts, [777], 200, 11)
    copies = rng.permutation([1] * 24 + [2] * 20 + [3] * 4)                      # 76 rows, so that 300 rows are left for the random strings
    seqs = [s for s, c in zip(wrap, copies) for _ in range(c)] + displaced + chain
    assert len(seqs) == 300
    seqs += [rng.randint(0, 256, 12).astype(np.uint8).tobytes() for _ in range(CHAIN_N - len(seqs))]
    seqs = [seqs[q] for q in rng.permutation(CHAIN_N)]
    return seqs, {"wrap": (wrap, [ts - 3, ts - 2, ts - 1]), "displaced": (displaced, [0, 1]), "chain": (chain, [777])}


@functools.lru_cache(None)
def order_cases():
    """inputs for the other id orders (first, zoned) on both sides of the scans' switch over n and over U"""
    out = {}
    for n, U in ((8191, 5000), (8192, 5000), (8193, 6000), (20000, 8100), (20000, 8192), (20000, 12353)):
        out["n%d_u%d" % (n, U)] = with_unique(np.random.RandomState(11000 + n + U), n, U)
    return out


@functools.lru_cache(None)
def all_plan_inputs():
    """every input of the plan tests, name -> seqs"""
    out = {k: v[0] for k, v in size_cases().items()}
    out.update(degenerate_cases())
    out.update(content_cases())
    out["probe_chains"] = probe_chain_case()[0]
    out.update(order_cases())
    return out
