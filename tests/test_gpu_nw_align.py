"""GPU tests of the alignment paths: nw_align on the host boundary, device.nw_align_pairs, and clusterconsensus on top of them.  ops, length,
matches and score are compared EXACTLY with the plain-Python full-matrix model (tests/nw_align_model.py, pinned against the oracle in
tests/test_nw_align_model.py); the shapes are the strip (32 columns) and decision-word (16 cells) boundaries, tie-heavy two-letter pairs,
all six matrices, penalties outside the combined-key range, and pair lists that put unlike shapes into one wavefront."""
import numpy as np
import pytest
import torch

import nw_align_model as model
import oracle_lib as O
from test_gpu_cross import bits, switches

pytestmark = pytest.mark.gpu

EDGE_LENGTHS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 96, 127]


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


def assert_aligned(da, x, y, pairs=None, matrix="BLOSUM62", go=10, ge=4, what=""):
    """nw_align(ops=True) and nw_align(ops=False) against the model, pair by pair"""
    px, py = (range(len(x)), range(len(y))) if pairs is None else pairs
    exp = [want(x[i], y[j], matrix, go, ge) for i, j in zip(px, py)]
    got = da.nw_align(x, y, matrix, go, ge, pairs=pairs)
    assert got.length.dtype == got.matches.dtype == got.score.dtype == np.int32
    assert len(got.ops) == len(got.length) == len(got.matches) == len(got.score) == len(exp), what
    for p, (ops, ln, mt, sc) in enumerate(exp):
        assert (got.ops[p], int(got.length[p]), int(got.matches[p]), int(got.score[p])) == (ops, ln, mt, sc), (what, "pair", p, len(x[px[p]]), len(y[py[p]]))
    ints = da.nw_align(x, y, matrix, go, ge, pairs=pairs, ops=False)
    assert ints.ops is None
    assert np.array_equal(ints.length, got.length) and np.array_equal(ints.matches, got.matches) and np.array_equal(ints.score, got.score), what
    return got


@pytest.mark.parametrize("a,b,matrix,go,ge,ops,ln,mt,sc", [
    ("YDYIHIYADKQDRIGWLGNT", "MYCEMNVEIQYMATKNMWNT", "BLOSUM62", 10, 4, "LDDDDDDDDDDDDDDDUDDDD", 21, 3, -17),
    ("MYCEMNVEIQYMATKNMWNT", "YDYIHIYADKQDRIGWLGNT", "BLOSUM62", 10, 4, "LDDDDDDDDDDDDDDDUDDDD", 21, 4, -17),
    ("PPPSYETVMAAA", "TPPPSYETVMAA", "BLOSUM62", 10, 4, "LDDDDDDDDDUDD", 13, 11, 35),
    ("ACACCA", "CAACAC", "BLOSUM45", 0, 0, "UDLDDLDU", None, None, None),
])
def test_known_answers(da, a, b, matrix, go, ge, ops, ln, mt, sc):
    r = da.nw_align([a], [b], matrix, go, ge)
    assert r.ops == [ops] and int(r.length[0]) == len(ops)
    if ln is not None:
        assert (int(r.length[0]), int(r.matches[0]), int(r.score[0])) == (ln, mt, sc)
    assert (r.ops[0], int(r.length[0]), int(r.matches[0]), int(r.score[0])) == want(a, b, matrix, go, ge)
    ga, gb = da.nw_align_strings(a, b, r.ops[0])
    assert (ga, gb) == model.gapped(a, b, ops) and sum(p == q for p, q in zip(ga, gb)) == int(r.matches[0])


@pytest.mark.parametrize("content", ["random", "mutated"])
def test_every_pair_of_strip_and_word_boundary_lengths(da, content):
    """11 x 11 lengths on both sides, through the NULL-list form (pair p is x[p] with y[p])"""
    rng = np.random.default_rng(31 if content == "random" else 32)
    x, y = [], []
    for la in EDGE_LENGTHS:
        for lb in EDGE_LENGTHS:
            a = model.random_seq(rng, la)
            if content == "random":
                b = model.random_seq(rng, lb)
            else:                                   # a mutated copy of a, cut or extended to lb residues
                b = model.mutate(rng, a)
                b = (b + model.random_seq(rng, max(lb - len(b), 0)))[:lb]
            x.append(a)
            y.append(b)
    assert len(x) == 121
    assert_aligned(da, x, y, what=content)


@pytest.mark.parametrize("go,ge", [(0, 0), (1, 1), (3, 0)])
def test_tie_heavy_two_letter_pairs(da, go, ge):
    rng = np.random.default_rng(77)
    x = [model.random_seq(rng, int(rng.integers(0, 41)), "AC") for _ in range(300)]
    y = [model.random_seq(rng, int(rng.integers(0, 41)), "AC") for _ in range(300)]
    got = assert_aligned(da, x, y, go=go, ge=ge, what="ties (%d, %d)" % (go, ge))
    assert len(set(got.ops)) > 100


@pytest.mark.parametrize("matrix", model.MATRICES)
def test_all_six_matrices(da, matrix):
    rng = np.random.default_rng(5)
    x = [model.random_seq(rng, int(rng.integers(0, 50)), model.ORDER) for _ in range(60)]
    y = [model.mutate(rng, s, model.ORDER) if t % 2 else model.random_seq(rng, int(rng.integers(0, 50)), model.ORDER) for t, s in enumerate(x)]
    assert_aligned(da, x, y, matrix=matrix, what=matrix)


def test_penalties_outside_the_combined_key_range(da):
    rng = np.random.default_rng(6)
    lens = [0, 1, 20, 33, 64, 127] + [int(v) for v in rng.integers(0, 60, 34)]
    x = [model.random_seq(rng, n) for n in lens]
    y = [model.mutate(rng, s) if t % 2 else model.random_seq(rng, lens[-1 - t]) for t, s in enumerate(x)]
    assert_aligned(da, x, y, go=200, ge=100, what="(200, 100)")


@pytest.fixture(scope="module")
def listed():
    """two pools of unlike lengths and 1000 (i, j) drawn with repeats, in no order: a wavefront holds lanes of every shape"""
    rng = np.random.default_rng(1000)
    lens = [0, 1, 2, 3, 5, 8, 12, 20, 20, 20, 20, 31, 32, 33, 40, 65, 96, 127] + [int(v) for v in rng.integers(4, 25, 30)]
    x = [model.random_seq(rng, n) for n in lens]
    y = [model.mutate(rng, x[int(rng.integers(0, len(x)))]) if t % 2 else model.random_seq(rng, n) for t, n in enumerate(lens)]
    px = rng.integers(0, len(x), 1000).astype(np.int32)
    py = rng.integers(0, len(y), 1000).astype(np.int32)
    return x, y, px, py


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257, 1000])
def test_pair_counts_through_index_lists(da, listed, count):
    x, y, px, py = listed
    assert_aligned(da, x, y, pairs=(px[:count], py[:count]), what="%d pairs" % count)


def test_several_blocks(da, listed):
    from dynaalign_amd import _capi
    x, y, px, py = listed
    block_bytes = 1 << 20
    per_pair = _capi.load().da_nw_align_workspace_bytes(64) // 64
    assert 1000 * per_pair >= 3 * block_bytes                # at least three blocks whatever the ops rows add
    with switches(DYNAALIGN_BLOCK_BYTES=str(block_bytes)):
        assert_aligned(da, x, y, pairs=(px, py), what="blocks")


def test_matches_and_length_equal_nw_pairs_on_the_evp_probes(da, evp):
    seqs = evp[:40]
    mt, ln, sc = da.nw_pairs(seqs)
    i, j = np.triu_indices(len(seqs))
    r = da.nw_align(seqs, seqs, pairs=(i, j), ops=False)
    assert np.array_equal(r.matches, mt[i, j]) and np.array_equal(r.length, ln[i, j]) and np.array_equal(r.score, sc[i, j])


def device_call(x, y, px, py, matrix="BLOSUM62", go=10, ge=4, work_pairs=None, ops=True):
    from dynaalign_amd import device
    dx, dy = device.DeviceSequences(*O.pack(x)), device.DeviceSequences(*O.pack(y))
    assert int(device.nw_encode(dx).item()) == 0 and int(device.nw_encode(dy).item()) == 0
    tx = None if px is None else torch.from_numpy(np.ascontiguousarray(px, np.int32)).cuda()
    ty = None if py is None else torch.from_numpy(np.ascontiguousarray(py, np.int32)).cuda()
    work = None if work_pairs is None else torch.empty(device.nw_align_workspace_bytes(work_pairs), dtype=torch.uint8, device="cuda")
    out = device.nw_align_pairs(dx, dy, matrix, go, ge, pair_x=tx, pair_y=ty, ops=ops, work=work)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in out]


@pytest.mark.parametrize("work_pairs", [None, 64])
def test_device_pointer_call_equals_the_host_call(da, listed, work_pairs):
    """... also with a workspace of one wavefront, which the call reuses launch after launch"""
    x, y, px, py = listed
    host = da.nw_align(x, y, pairs=(px, py))
    ops, ln, mt, sc = device_call(x, y, px, py, work_pairs=work_pairs)
    assert np.array_equal(ln, host.length) and np.array_equal(mt, host.matches) and np.array_equal(sc, host.score)
    assert ops.shape[0] == 1000 and ops.dtype == np.uint8
    for p in range(1000):
        assert ops[p, :ln[p]].tobytes().decode() == host.ops[p] and not ops[p, ln[p]:].any(), p
    ints = device_call(x, y, px, py, ops=False)
    assert ints[0] is None and np.array_equal(ints[1], ln) and np.array_equal(ints[2], mt) and np.array_equal(ints[3], sc)


def test_device_pointer_call_without_lists_and_with_a_pair_it_cannot_take(da):
    x, y = ["ACDEF", "", "WWKK"], ["ACDF", "KK", ""]
    ops, ln, mt, sc = device_call(x, y, None, None)
    host = da.nw_align(x, y)
    assert np.array_equal(ln, host.length) and np.array_equal(mt, host.matches) and np.array_equal(sc, host.score)
    assert [ops[p, :ln[p]].tobytes().decode() for p in range(3)] == host.ops
    # the lists live on the device: an index outside its set is reported per pair, not refused
    ops, ln, mt, sc = device_call(x, y, [0, 3, 2, -1], [0, 0, 5, 0])
    assert ln.tolist() == [int(host.length[0]), -1, -1, -1] and mt.tolist()[1:] == [-1, -1, -1] and sc.tolist()[1:] == [0, 0, 0]
    assert not ops[1:].any()


def test_aligning_the_top_k_hits_gives_their_values_bit_for_bit(da):
    from dynaalign_amd import synth
    seqs = synth.to_strings(*synth.h3n2_like(250, 20))
    rng = np.random.default_rng(9)
    x = [model.mutate(rng, s) or "A" for s in seqs[:50]]
    y = seqs[50:]
    idx, val = da.similarityNW_cross_topk(x, y, top=5)
    assert idx.shape == (50, 5)
    r = da.nw_align(x, y, pairs=(np.repeat(np.arange(50), 5), idx.ravel()), ops=False)
    assert np.array_equal(bits(r.matches / r.length), bits(val.ravel()))


def consensus_rows():
    rng = np.random.default_rng(2026)
    rows = []
    for c in range(30):
        root = model.random_seq(rng, 20)
        for _ in range(1 + c % 12):
            rows.append((model.mutate(rng, root, rate=0.2), "c%d" % c))
    order = rng.permutation(len(rows))             # members of a cluster are not adjacent
    return [rows[t] for t in order]


def test_clusterconsensus_equals_the_model(da):
    rows = consensus_rows()
    sizes = {}
    for _, cid in rows:
        sizes[cid] = sizes.get(cid, 0) + 1
    assert len(sizes) == 30 and set(sizes.values()) == set(range(1, 13))
    got = da.clusterconsensus(rows)
    assert got == model.consensus(rows, aligner=want)
    assert got == da.clusterconsensus(np.array(rows, dtype=object))


def test_clusterconsensus_on_a_clusterbreak_result(da):
    from dynaalign_amd import synth
    seqs = synth.to_strings(*synth.h3n2_like(600, 20))
    res = da.clusterbreak(seqs, thresh_p=0.8, size_max=30, size_min=3, sim_fn=lambda s: da.similarityNW(s), cluster_seed=3)
    labels = list(res["clustered_seq"][:, 1])
    ids = list(dict.fromkeys(labels))
    assert len(ids) > 1
    cons = da.clusterconsensus(res["clustered_seq"])
    assert [c[0] for c in cons] == ids
    assert all(0 < len(c[1]) <= 20 and set(c[1]) <= set(model.ORDER) for c in cons)
    assert da.clusterconsensus(res) == cons
