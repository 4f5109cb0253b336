"""GPU tests of the alignment paths of sequences up to 1024 residues: nw_align_long on the host boundary, device.nw_align_long_pairs, and
clusterconsensus(align_fn=nw_align_long).  ops, length, matches and score are compared EXACTLY with the plain-Python full-matrix model
(tests/nw_align_model.py, pinned above 127 residues in tests/test_nw_align_long_model.py); every case also runs with ops=False and must give
the same integers.  The shapes are the lane-ownership boundaries of the wavefront-per-pair kernel (sequence2 of 64 W and 64 W + 1 residues
for every width W), fewer and more rows than lanes, empty sides, tie-heavy two-letter pairs, all six matrices, large penalties, lists that
mix both kernels, slot reuse, and several host blocks.  The model costs a few microseconds per cell: the shapes keep each test to seconds."""
import numpy as np
import pytest
import torch

import nw_align_model as model
import oracle_lib as O
from test_gpu_cross import bits, switches

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 3, 4, 6, 8, 9, 12, 16]
OWNERSHIP_LENGTHS = [128, 129, 192, 193, 256, 257, 384, 385, 512, 513, 576, 577, 768, 769, 1023, 1024]


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    from dynaalign_amd import _capi
    assert _capi.load().da_device_count() > 0
    return dynaalign_amd


_CACHE = {}


def want(a, b, matrix="BLOSUM62", go=10, ge=4):
    key = (a, b, matrix, go, ge)
    if key not in _CACHE:
        _CACHE[key] = model.align(a, b, matrix, go, ge)
    return _CACHE[key]


def mutated(rng, a, lb, alphabet=model.ORDER[:20]):
    """a mutated copy of a, cut or extended to lb residues"""
    b = model.mutate(rng, a, alphabet, max_len=4096)
    return (b + model.random_seq(rng, max(lb - len(b), 0), alphabet))[:lb]


def assert_aligned(da, x, y, pairs=None, matrix="BLOSUM62", go=10, ge=4, what=""):
    """nw_align_long(ops=True) and nw_align_long(ops=False) against the model, pair by pair"""
    px, py = (range(len(x)), range(len(y))) if pairs is None else pairs
    exp = [want(x[i], y[j], matrix, go, ge) for i, j in zip(px, py)]
    got = da.nw_align_long(x, y, matrix, go, ge, pairs=pairs)
    assert got.length.dtype == got.matches.dtype == got.score.dtype == np.int32
    assert len(got.ops) == len(got.length) == len(got.matches) == len(got.score) == len(exp), what
    for p, (ops, ln, mt, sc) in enumerate(exp):
        assert (int(got.length[p]), int(got.matches[p]), int(got.score[p])) == (ln, mt, sc), (what, "pair", p, len(x[px[p]]), len(y[py[p]]))
        assert got.ops[p] == ops, (what, "pair", p, len(x[px[p]]), len(y[py[p]]))
    ints = da.nw_align_long(x, y, matrix, go, ge, pairs=pairs, ops=False)
    assert ints.ops is None
    assert np.array_equal(ints.length, got.length) and np.array_equal(ints.matches, got.matches) and np.array_equal(ints.score, got.score), what
    return got


def test_the_ownership_lengths_are_64_w_and_64_w_plus_1_of_every_width():
    assert sorted(OWNERSHIP_LENGTHS) == sorted([64 * w for w in WIDTHS[1:]] + [64 * w + 1 for w in WIDTHS[1:-1]] + [1023])


@pytest.mark.parametrize("content", ["random", "mutated"])
def test_lane_ownership_boundaries(da, content):
    """sequence2 of 64 W and 64 W + 1 residues for every width; sequence1 of 1 and 33 residues: fewer rows than active lanes, and more"""
    rng = np.random.default_rng(41 if content == "random" else 42)
    x, y = [], []
    for lb in OWNERSHIP_LENGTHS:
        for la in (1, 33):
            b = model.random_seq(rng, lb)
            a = model.random_seq(rng, la) if content == "random" else mutated(rng, b[lb // 2:], la)
            x.append(a)
            y.append(b)
    assert len(x) == 32
    assert_aligned(da, x, y, what=content)


def test_long_rows_few_columns(da):
    rng = np.random.default_rng(43)
    x, y = [], []
    for la in (128, 129, 566, 1023, 1024):
        for lb in (1, 2, 17, 65, 127):
            a = model.random_seq(rng, la)
            x.append(a)
            y.append(mutated(rng, a[la // 3:], lb) if (la + lb) % 2 else model.random_seq(rng, lb))
    assert_aligned(da, x, y, what="long rows")


def test_empty_sides_in_a_list_with_long_pairs(da):
    rng = np.random.default_rng(44)
    shapes = [(200, 150), (0, 128), (128, 0), (130, 140), (0, 1024), (1024, 0), (0, 0), (129, 5)]
    x = [model.random_seq(rng, la) for la, _ in shapes]
    y = [model.random_seq(rng, lb) for _, lb in shapes]
    got = assert_aligned(da, x, y, what="empty sides")
    assert got.ops[1] == "L" * 128 and got.ops[2] == "U" * 128 and got.ops[4] == "L" * 1024 and got.ops[5] == "U" * 1024 and got.ops[6] == ""
    assert got.score.tolist()[4:7] == [model.NEG, model.NEG, 0]


def test_both_long(da):
    rng = np.random.default_rng(45)
    a = model.random_seq(rng, 566)
    c = model.random_seq(rng, 640)
    x = [a, model.random_seq(rng, 567), c]
    y = [mutated(rng, a, 566), model.random_seq(rng, 566), mutated(rng, c, 600)]
    assert_aligned(da, x, y, what="both long")


def test_1024_by_1024(da):
    rng = np.random.default_rng(46)
    a = model.random_seq(rng, 1024)
    assert_aligned(da, [a], [mutated(rng, a, 1024)], what="1024 x 1024")
    assert_aligned(da, [model.random_seq(rng, 1024, "AC")], [model.random_seq(rng, 200, "AC")], go=0, ge=0, what="1024 x 200, two letters")


@pytest.mark.parametrize("go,ge", [(0, 0), (1, 1), (3, 0)])
def test_tie_heavy_two_letter_pairs(da, go, ge):
    rng = np.random.default_rng(77)
    x = [model.random_seq(rng, int(rng.integers(128, 221)), "AC") for _ in range(16)]
    y = [model.random_seq(rng, int(rng.integers(128, 221)), "AC") for _ in range(16)]
    got = assert_aligned(da, x, y, go=go, ge=ge, what="ties (%d, %d)" % (go, ge))
    assert len(set(got.ops)) > 10


@pytest.mark.parametrize("matrix", model.MATRICES)
def test_all_six_matrices(da, matrix):
    rng = np.random.default_rng(5)
    x = [model.random_seq(rng, int(rng.integers(130, 201)), model.ORDER) for _ in range(6)]
    y = [mutated(rng, s, int(rng.integers(130, 201)), model.ORDER) if t % 2 else model.random_seq(rng, int(rng.integers(130, 201)), model.ORDER)
         for t, s in enumerate(x)]
    assert_aligned(da, x, y, matrix=matrix, what=matrix)


def test_penalties_200_100(da):
    rng = np.random.default_rng(6)
    shapes = [(128, 300), (300, 128), (150, 150), (129, 20), (20, 129), (200, 190), (0, 130), (140, 257)]
    x = [model.random_seq(rng, la) for la, _ in shapes]
    y = [mutated(rng, s, shapes[t][1]) if t % 2 == 0 else model.random_seq(rng, shapes[t][1]) for t, s in enumerate(x)]
    assert_aligned(da, x, y, go=200, ge=100, what="(200, 100)")


def test_mixed_list_keeps_the_listed_order(da):
    """pairs for the lane-per-pair kernels and for the wavefront kernel in one list, drawn with repeats"""
    rng = np.random.default_rng(1001)
    lens = [0, 1, 20, 20, 64, 127, 128, 200, 300]
    x = [model.random_seq(rng, n) for n in lens]
    y = [mutated(rng, x[int(rng.integers(0, len(x)))], n) if t % 2 else model.random_seq(rng, n) for t, n in enumerate(lens)]
    px = rng.integers(0, len(x), 600).astype(np.int32)
    py = rng.integers(0, len(y), 600).astype(np.int32)
    got = assert_aligned(da, x, y, pairs=(px, py), what="mixed")
    short = np.array([len(x[i]) <= 127 and len(y[j]) <= 127 for i, j in zip(px, py)])
    assert 100 < short.sum() < 500
    ref = da.nw_align(x, y, pairs=(px[short], py[short]))
    assert ref.ops == [got.ops[p] for p in np.flatnonzero(short)]
    assert np.array_equal(ref.length, got.length[short]) and np.array_equal(ref.matches, got.matches[short]) and np.array_equal(ref.score, got.score[short])


def test_short_only_inputs_equal_nw_align(da):
    """the `listed` inputs of tests/test_gpu_nw_align.py, regenerated from the same seed: every pair goes to the lane-per-pair kernels"""
    rng = np.random.default_rng(1000)
    lens = [0, 1, 2, 3, 5, 8, 12, 20, 20, 20, 20, 31, 32, 33, 40, 65, 96, 127] + [int(v) for v in rng.integers(4, 25, 30)]
    x = [model.random_seq(rng, n) for n in lens]
    y = [model.mutate(rng, x[int(rng.integers(0, len(x)))]) if t % 2 else model.random_seq(rng, n) for t, n in enumerate(lens)]
    px = rng.integers(0, len(x), 1000).astype(np.int32)
    py = rng.integers(0, len(y), 1000).astype(np.int32)
    for ops in (True, False):
        a, b = da.nw_align_long(x, y, pairs=(px, py), ops=ops), da.nw_align(x, y, pairs=(px, py), ops=ops)
        assert a.ops == b.ops and np.array_equal(a.length, b.length) and np.array_equal(a.matches, b.matches) and np.array_equal(a.score, b.score)
    a, b = da.nw_align_long(x[:40], y[:40]), da.nw_align(x[:40], y[:40])       # the NULL-list form
    assert a.ops == b.ops and np.array_equal(a.length, b.length) and np.array_equal(a.matches, b.matches) and np.array_equal(a.score, b.score)


def device_call(x, y, px, py, work_bytes=None, ops=True, **kw):
    from dynaalign_amd import device
    dx, dy = device.DeviceSequences(*O.pack(x)), device.DeviceSequences(*O.pack(y))
    assert int(device.nw_encode(dx).item()) == 0 and int(device.nw_encode(dy).item()) == 0
    tx = None if px is None else torch.from_numpy(np.ascontiguousarray(px, np.int32)).cuda()
    ty = None if py is None else torch.from_numpy(np.ascontiguousarray(py, np.int32)).cuda()
    work = None if work_bytes is None else torch.empty(work_bytes, dtype=torch.uint8, device="cuda")
    out = device.nw_align_long_pairs(dx, dy, pair_x=tx, pair_y=ty, ops=ops, work=work, **kw)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in out]


@pytest.fixture(scope="module")
def forty():
    rng = np.random.default_rng(1002)
    lens = [300, 0, 1, 64, 65, 127, 128, 129, 200, 257, 299, 33]
    x = [model.random_seq(rng, n) for n in lens]
    y = [mutated(rng, x[int(rng.integers(0, len(x)))], n) if t % 2 else model.random_seq(rng, n) for t, n in enumerate(reversed(lens))]
    px = rng.integers(0, len(x), 40).astype(np.int32)
    py = rng.integers(0, len(y), 40).astype(np.int32)
    return x, y, px, py


def test_slot_reuse_one_slot_equals_the_default_workspace_equals_the_host_call(da, forty):
    from dynaalign_amd import device
    x, y, px, py = forty
    host = assert_aligned(da, x, y, pairs=(px, py), what="forty")
    one = device.nw_align_long_workspace_bytes(1, 300)
    assert one == (300 + 63) * 256 and device.nw_align_long_workspace_bytes(40, 300) == 40 * one
    for work_bytes in (one, None):
        ops, ln, mt, sc = device_call(x, y, px, py, work_bytes=work_bytes)
        assert np.array_equal(ln, host.length) and np.array_equal(mt, host.matches) and np.array_equal(sc, host.score), work_bytes
        assert ops.shape == (40, 600) and ops.dtype == np.uint8
        for p in range(40):
            assert ops[p, :ln[p]].tobytes().decode() == host.ops[p] and not ops[p, ln[p]:].any(), (work_bytes, p)
    ints = device_call(x, y, px, py, ops=False)                      # no workspace at all
    assert ints[0] is None and np.array_equal(ints[1], host.length) and np.array_equal(ints[2], host.matches) and np.array_equal(ints[3], host.score)


def test_pairs_the_kernel_cannot_take_are_reported_per_pair(da, forty):
    x, y, px, py = forty
    host = da.nw_align_long(x, y, pairs=(px, py))
    lx, ly = np.array([len(s) for s in x])[px], np.array([len(s) for s in y])[py]

    def check(out, bad, ops_wanted=True):
        ops, ln, mt, sc = out
        assert 0 < bad.sum() < len(bad)
        assert (ln[bad] == -1).all() and (mt[bad] == -1).all() and (sc[bad] == 0).all()
        assert np.array_equal(ln[~bad], host.length[~bad]) and np.array_equal(mt[~bad], host.matches[~bad]) and np.array_equal(sc[~bad], host.score[~bad])
        if ops_wanted:
            assert not ops[bad].any()
            for p in np.flatnonzero(~bad):
                assert ops[p, :ln[p]].tobytes().decode() == host.ops[p] and not ops[p, ln[p]:].any(), p

    # an index outside its set
    bx, by = px.copy(), py.copy()
    bx[[3, 17]] = [len(x), -1]
    by[[5, 39]] = [len(y) + 7, -2 ** 31]
    bad = np.zeros(40, bool)
    bad[[3, 17, 5, 39]] = True
    check(device_call(x, y, bx, by), bad)
    check(device_call(x, y, bx, by, ops=False), bad, ops_wanted=False)
    # a sequence over max_len
    bad = (lx > 200) | (ly > 200)
    check(device_call(x, y, px, py, max_len=200), bad)
    check(device_call(x, y, px, py, max_len=200, ops=False), bad, ops_wanted=False)
    # an ops row too short for the pair: only with ops
    bad = lx + ly > 350
    check(device_call(x, y, px, py, ld_ops=350), bad)
    ints = device_call(x, y, px, py, ld_ops=350, ops=False)
    assert np.array_equal(ints[1], host.length)


def test_several_host_blocks(da):
    rng = np.random.default_rng(1003)
    lens = [0, 1, 5, 20, 20, 33, 64, 127, 300, 400]
    x = [model.random_seq(rng, n) for n in lens]
    y = [mutated(rng, x[int(rng.integers(0, len(x)))], n) if t % 2 else model.random_seq(rng, n) for t, n in enumerate(lens)]
    px = rng.integers(0, len(x), 3000).astype(np.int32)
    py = rng.integers(0, len(y), 3000).astype(np.int32)
    block_bytes = 1 << 20
    longest = max(len(x[i]) + len(y[j]) for i, j in zip(px, py))
    is_long = np.array([len(x[i]) > 127 or len(y[j]) > 127 for i, j in zip(px, py)])
    assert 3000 * longest > 2 * block_bytes and 700 < is_long.sum() < 2300          # the ops rows alone exceed two blocks; both kernels get many pairs
    with switches(DYNAALIGN_BLOCK_BYTES=str(block_bytes)):
        assert_aligned(da, x, y, pairs=(px, py), what="blocks")


def test_ha_sized_pairs_against_the_similarity_calls(da):
    """no model here: 24 sequences of 566 residues, all 576 ordered pairs, against similarityNW_cross and nw_pairs"""
    from dynaalign_amd import synth
    seqs = synth.to_strings(*synth.h3n2_like(24, 566))
    assert {len(s) for s in seqs} == {566}
    i, j = (v.ravel() for v in np.meshgrid(np.arange(24), np.arange(24), indexing="ij"))
    r = da.nw_align_long(seqs, seqs, pairs=(i, j))
    ints = da.nw_align_long(seqs, seqs, pairs=(i, j), ops=False)
    assert np.array_equal(ints.length, r.length) and np.array_equal(ints.matches, r.matches) and np.array_equal(ints.score, r.score)
    cross = da.similarityNW_cross(seqs, seqs)
    assert np.array_equal(bits(r.matches / r.length), bits(cross.ravel()))
    mt, ln, sc = da.nw_pairs(seqs)
    up = i <= j
    assert np.array_equal(r.matches[up], mt[i[up], j[up]]) and np.array_equal(r.length[up], ln[i[up], j[up]]) and np.array_equal(r.score[up], sc[i[up], j[up]])
    for p in range(576):
        ops, a, b = r.ops[p], seqs[i[p]], seqs[j[p]]
        assert len(ops) == int(r.length[p]) and set(ops) <= set("DUL")
        ia = ib = same = 0
        for op in ops:
            same += op == "D" and a[ia] == b[ib]
            ia += op != "L"
            ib += op != "U"
        assert (ia, ib) == (566, 566) and same == int(r.matches[p]), p


def consensus_rows():
    rng = np.random.default_rng(2027)
    rows = []
    for c in range(1, 5):                                          # clusters of 1, 2, 3 and 4 mutated 130 .. 160-mers
        root = model.random_seq(rng, int(rng.integers(142, 153)))
        for _ in range(c):
            rows.append((model.mutate(rng, root, max_len=160), "long%d" % c))
    root = model.random_seq(rng, 20)
    rows += [(model.mutate(rng, root, rate=0.2), "short") for _ in range(5)]
    order = rng.permutation(len(rows))                             # members of a cluster are not adjacent
    return [rows[t] for t in order]


def test_clusterconsensus_with_nw_align_long_equals_the_model(da):
    rows = consensus_rows()
    sizes = {}
    for _, cid in rows:
        sizes[cid] = sizes.get(cid, 0) + 1
    assert sorted(sizes.values()) == [1, 2, 3, 4, 5]
    assert all(130 <= len(s) <= 160 for s, cid in rows if cid != "short") and all(len(s) <= 30 for s, cid in rows if cid == "short")
    got = da.clusterconsensus(rows, align_fn=da.nw_align_long)
    assert got == model.consensus(rows, aligner=want)
    with pytest.raises(da.DynaAlignError):                         # the default call still stops at 127 residues
        da.clusterconsensus(rows)
