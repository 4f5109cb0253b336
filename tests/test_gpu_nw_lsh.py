"""GPU tests of the NW identity on MinHash LSH candidates (nw_lsh_kernels.hip): the host entries similarityNW_lsh_edges /
similarityNW_lsh_cross_edges, the device pieces device.nw_rescore_pairs / device.lsh_nw_edges, and clusterbreak on the graph.  Every
comparison is exact -- indices as integers, weights as uint64 bit patterns.  The expected values come from the oracle's pair value on the
candidates of the LSH model of test_lsh_cpu.py over the oracle's signatures, never from the code under test."""
import numpy as np
import pytest
import torch

import oracle_lib as O
from test_gpu_jaccard import family
from test_lsh_cpu import model
from test_lsh_cross_cpu import cross_model
from test_nw_lsh_cpu import AA20, nw_model, same_edges

pytestmark = pytest.mark.gpu

SEED = 12345
UNSUPPORTED = 10
N_HASH = 48
BANDINGS = [(12, 4), (40, 1)]


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    from dynaalign_amd import _capi
    assert _capi.load().da_device_count() > 0
    return dynaalign_amd


def oracle_sig(seqs, k=4, n_hash=N_HASH):
    return O.signatures(seqs, k, n_hash, O.seeds(SEED, n_hash))


class PairValues:
    """the oracle's (matches, length) of x[i] as sequence1 against y[j] as sequence2, each pair computed once"""

    def __init__(self, x, y, go=10, ge=4):
        self.x, self.y, self.go, self.ge, self.seen = x, y, go, ge, {}

    def ml(self, i, j):
        if (i, j) not in self.seen:
            rc, mt, ln, _, _ = O.nw_pair(self.x[i], self.y[j], "BLOSUM62", self.go, self.ge)
            assert rc == 0
            self.seen[(i, j)] = (mt, ln)
        return self.seen[(i, j)]

    def __call__(self, i, j):
        mt, ln = self.ml(i, j)
        return mt / ln


def rand_seq(rng, length):
    return "".join(AA20[t] for t in rng.randint(0, 20, length))


def short_set():
    """family() 20-mers plus planted pairs of a 20-mer and its first 10 / first 9 residues: identity exactly 10 / 20 and 9 / 20"""
    rng = np.random.RandomState(99)
    seqs = family(11, 6, 20, 200)
    for _ in range(40):
        p = rand_seq(rng, 20)
        seqs += [p, p[:10], p[:9]]
    return list(dict.fromkeys(seqs))


@pytest.fixture(scope="module")
def short_case():
    seqs = short_set()
    return seqs, oracle_sig(seqs), PairValues(seqs, seqs)


@pytest.mark.parametrize("thr", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("mh_thr", [0.0, 0.5])
@pytest.mark.parametrize("bands,rows", BANDINGS, ids=["12x4", "40x1"])
def test_host_entry_equals_the_model(da, short_case, bands, rows, mh_thr, thr):
    """A value below 0.0 does not exist, so `just below the threshold` is asked of 0.5 and 1.0 only; at 0.0 a candidate under 0.5 must be
    kept.  The pre-filter can only drop a pair when mh_threshold > 0."""
    seqs, sig, value = short_case
    assert 200 <= len(seqs) <= 400
    cand = model(sig, bands, rows, mh_thr)
    want = nw_model(cand["i"], cand["j"], value, thr)
    # what the inputs were chosen for
    values = np.array(list(want["all"].values()))
    assert len(cand["i"]) > len(seqs)
    if thr > 0:
        assert (values == thr).any() and ((values < thr) & (values >= thr - 0.1)).any()
    else:
        assert ((values > 0) & (values < 0.5)).any()
    dropped = model(sig, bands, rows, 0.0)["pairs"] - set(zip(cand["i"], cand["j"]))
    if mh_thr > 0:
        assert len(dropped) > 0
    got_thr, i, j, w = da.similarityNW_lsh_edges(seqs, 4, N_HASH, bands, rows, thr, mh_threshold=mh_thr, seed=SEED)
    assert got_thr == thr
    same_edges((i, j, w), want)
    assert not (set(zip(i.tolist(), j.tolist())) & dropped)
    route = da.nw_lsh_last_route()
    assert route["aligned_pairs"] == len(cand["i"]) == route["short_pairs"] and route["long_pairs"] == 0 and route["edges"] == len(i)
    assert route["verified_pairs"] == len(model(sig, bands, rows, 0.0)["pairs"])


# ---- device.nw_rescore_pairs on synthetic lists ----------------------------------------------------------------------------------------------
LENGTHS = [1, 32, 33, 127, 128, 129, 1024]


@pytest.fixture(scope="module")
def length_sets(da):
    """x and y: one sequence of every length at which a kernel takes another path, then an empty one and one of 1025 residues (refused)"""
    from dynaalign_amd import device
    rng = np.random.RandomState(5)
    base = rand_seq(rng, 1024)
    x = [base[:n] for n in LENGTHS] + ["", rand_seq(rng, 1025)]
    y = []
    for n in LENGTHS:                                # relatives of x's sequences: a few substitutions, so that matches are not trivial
        s = list(base[:n])
        for _ in range(max(n // 10, 1)):
            s[rng.randint(0, n)] = AA20[rng.randint(0, 20)]
        y.append("".join(s))
    y += ["", rand_seq(rng, 1025)]
    dx, dy = device.DeviceSequences(*O.pack(x)), device.DeviceSequences(*O.pack(y))
    device.nw_encode(dx)
    device.nw_encode(dy)
    return x, y, dx, dy, PairValues(x, y)


SHORT = [(a, b) for a in range(4) for b in range(4)]
LONG = [(a, b) for a in range(7) for b in range(7) if a >= 4 or b >= 4]


def listed(layout, count):
    s = [SHORT[p % len(SHORT)] for p in range(count)]
    g = [LONG[p % len(LONG)] for p in range(count)]
    if layout == "short":
        return s
    if layout == "long":
        return g
    if layout == "alternating":
        return [s[p] if p % 2 == 0 else g[p] for p in range(count)]
    if layout == "long_first":
        return [LONG[0]] * min(count, 1) + s[1:]
    assert layout == "long_last"
    return s[:-1] + [LONG[3]] * min(count, 1)


def rescore(device, dx, dy, pairs, **kw):
    i = torch.tensor([p[0] for p in pairs], dtype=torch.int32, device="cuda")
    j = torch.tensor([p[1] for p in pairs], dtype=torch.int32, device="cuda")
    mt, ln = device.nw_rescore_pairs(dx, dy, i, j, **kw)
    torch.cuda.synchronize()
    return mt.cpu().tolist(), ln.cpu().tolist()


@pytest.mark.parametrize("layout", ["short", "long", "alternating", "long_first", "long_last"])
def test_rescore_pairs_on_synthetic_lists(da, length_sets, layout):
    from dynaalign_amd import device
    x, y, dx, dy, value = length_sets
    assert len(LONG) == 33 and len(SHORT) == 16              # the oracle aligns every distinct pair once: 33 with a side over 127 residues
    for count in (0, 1, 63, 64, 65, 4097):
        pairs = listed(layout, count)
        mt, ln = rescore(device, dx, dy, pairs)
        assert (mt, ln) == ([value.ml(*p)[0] for p in pairs], [value.ml(*p)[1] for p in pairs]), (layout, count)
        route = device.nw_lsh_last_route()
        longs = sum(1 for a, b in pairs if a >= 4 or b >= 4)
        assert (route["aligned_pairs"], route["short_pairs"], route["long_pairs"]) == (count, count - longs, longs)


def test_rescore_refuses_pair_by_pair(da, length_sets):
    from dynaalign_amd import device
    x, y, dx, dy, value = length_sets
    bad = [(-1, 0), (9, 0), (0, -1), (0, 9), (7, 0), (0, 7), (8, 2), (5, 8), (7, 8), (2 ** 31 - 1, 0)]   # outside x / y, empty, 1025 residues
    pairs = []
    for p, b in enumerate(bad * 7):                           # a refused pair at every position of a chunk's class pattern
        pairs += [b, SHORT[p % 16], LONG[p % 33]][:1 + p % 3]
    pairs += bad
    mt, ln = rescore(device, dx, dy, pairs)
    for p, (a, b) in enumerate(pairs):
        want = (-1, -1) if (a, b) in bad else value.ml(a, b)
        assert (mt[p], ln[p]) == want, (p, a, b)
    only_bad = rescore(device, dx, dy, bad)
    assert only_bad == ([-1] * len(bad), [-1] * len(bad))
    route = device.nw_lsh_last_route()
    assert (route["aligned_pairs"], route["short_pairs"], route["long_pairs"]) == (len(bad), 0, 0)


def test_rescore_workspace_of_any_alignment_and_the_minimal_one(da, length_sets):
    from dynaalign_amd import device
    x, y, dx, dy, value = length_sets
    pairs = listed("alternating", 4097)
    want = ([value.ml(*p)[0] for p in pairs], [value.ml(*p)[1] for p in pairs])
    full_b, min_b = device.nw_rescore_workspace_bytes(len(pairs)), device.nw_rescore_workspace_bytes(len(pairs), minimal=True)
    assert min_b < full_b
    full = torch.empty(full_b + 4, dtype=torch.uint8, device="cuda")
    assert full.data_ptr() % 256 == 0
    assert rescore(device, dx, dy, pairs, work=full[4:]) == want             # 4 bytes off alignment
    small = torch.empty(min_b + 4, dtype=torch.uint8, device="cuda")
    assert rescore(device, dx, dy, pairs, work=small[4:]) == want            # one wavefront of short pairs in flight: 33 launches
    assert rescore(device, dx, dy, pairs, work=small[:min_b]) == want
    with pytest.raises(da.DynaAlignError) as e:
        rescore(device, dx, dy, pairs, work=small[:min_b - 1])
    assert "workspace too small" in str(e.value)


# ---- mixed lengths in one call ---------------------------------------------------------------------------------------------------------------
def mixed_set():
    """200 short peptides, 12 sequences of 300 .. 600 residues derived from 3 parents, and 20-mers cut out of those parents: short pairs, long
    pairs and pairs of a short and a long sequence in one candidate list"""
    rng = np.random.RandomState(17)
    seqs = family(21, 5, 20, 260)
    for length in (300, 450, 600):
        parent = rand_seq(rng, length)
        for _ in range(4):
            s = list(parent)
            for _ in range(length // 25):
                s[rng.randint(0, len(s))] = AA20[rng.randint(0, 20)]
            cut = rng.randint(0, 8)
            seqs.append("".join(s)[cut:])
        seqs += [parent[a:a + 20] for a in (0, 100, 200)]
    return list(dict.fromkeys(seqs))


@pytest.fixture(scope="module")
def mixed_case():
    seqs = mixed_set()
    return seqs, oracle_sig(seqs), PairValues(seqs, seqs)


def test_mixed_lengths_in_one_call(da, mixed_case):
    seqs, sig, value = mixed_case
    lens = np.array([len(s) for s in seqs])
    assert (lens <= 127).sum() >= 200 and ((lens >= 300 - 8) & (lens <= 600)).sum() == 12
    cand = model(sig, 40, 1, 0.0)
    kinds = {int(lens[i] > 127) + int(lens[j] > 127) for i, j in zip(cand["i"], cand["j"])}
    assert kinds == {0, 1, 2}                                # short-short, short-long and long-long candidates
    n_long = sum(1 for i, j in zip(cand["i"], cand["j"]) if max(lens[i], lens[j]) > 127)
    assert 12 < n_long < 300                                 # what the CPU oracle aligns in a second
    want = nw_model(cand["i"], cand["j"], value, 0.5)
    _, i, j, w = da.similarityNW_lsh_edges(seqs, 4, N_HASH, 40, 1, 0.5, seed=SEED)
    same_edges((i, j, w), want)
    route = da.nw_lsh_last_route()
    assert route["short_pairs"] == len(cand["i"]) - n_long > 0 and route["long_pairs"] == n_long > 0
    assert route["aligned_pairs"] == len(cand["i"]) and route["edges"] == len(i) and route["buckets"] > 0 and route["incidences"] > 0


def test_several_blocks_give_the_same_list(da, mixed_case, monkeypatch):
    seqs, sig, value = mixed_case
    cand = model(sig, 40, 1, 0.0)
    want = nw_model(cand["i"], cand["j"], value, 0.5)
    monkeypatch.setenv("DYNAALIGN_BLOCK_BYTES", str(1 << 20))   # three wavefronts of short pairs in flight: the candidates take many launches
    assert len(cand["i"]) > 10 * 192
    _, i, j, w = da.similarityNW_lsh_edges(seqs, 4, N_HASH, 40, 1, 0.5, seed=SEED)
    same_edges((i, j, w), want)


def test_the_diagonal_is_scored(da):
    seqs = ["X" * 10, "X" * 20, "ACDEFGHIKLMNPQRSTVWY", "ACDEFGHIKLMNPQRSTVWA", "X" * 9 + "A"]
    value = PairValues(seqs, seqs, 0, 0)
    sig = oracle_sig(seqs)
    cand = model(sig, 12, 4, 0.0)
    want = nw_model(cand["i"], cand["j"], value, 0.5)
    assert value(0, 0) < 0.5 and value(1, 1) < 0.5 and value(2, 2) == 1.0
    _, i, j, w = da.similarityNW_lsh_edges(seqs, 4, N_HASH, 12, 4, 0.5, gapOpen=0, gapExt=0, seed=SEED)
    same_edges((i, j, w), want)
    edges = set(zip(i.tolist(), j.tolist()))
    assert (0, 0) not in edges and (1, 1) not in edges and (2, 2) in edges


# ---- two sets --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cross_case():
    seqs = mixed_set()
    rng = np.random.RandomState(3)
    order = rng.permutation(len(seqs))
    x = [seqs[t] for t in order[:60]] + [s for s in seqs if len(s) > 127][:6]
    y = [seqs[t] for t in order[40:]]
    return x, y, oracle_sig(x), oracle_sig(y)


def test_two_sets_against_the_model_and_sequence1_is_x(da, cross_case):
    x, y, sx, sy = cross_case
    assert any(len(s) > 127 for s in x) and any(len(s) <= 127 for s in x) and any(len(s) > 127 for s in y) and any(len(s) <= 127 for s in y)
    xy, yx = PairValues(x, y), PairValues(y, x)
    cand = cross_model(sx, sy, 40, 1, 0.0)
    want = nw_model(cand["i"], cand["j"], xy, 0.121)
    assert 0 < len(want["i"]) < len(cand["i"])
    _, i, j, w = da.similarityNW_lsh_cross_edges(x, y, 4, N_HASH, 40, 1, 0.121, seed=SEED)
    same_edges((i, j, w), want)
    route = da.nw_lsh_last_route()
    assert route["short_pairs"] > 0 and route["long_pairs"] > 0 and route["aligned_pairs"] == len(cand["i"])
    # the swapped call: the same pairs transposed, and a weight differs exactly where the oracle's value depends on the order
    cand_t = cross_model(sy, sx, 40, 1, 0.0)
    assert set(zip(cand_t["j"], cand_t["i"])) == set(zip(cand["i"], cand["j"]))
    want_t = nw_model(cand_t["i"], cand_t["j"], yx, 0.121)
    _, ti, tj, tw = da.similarityNW_lsh_cross_edges(y, x, 4, N_HASH, 40, 1, 0.121, seed=SEED)
    same_edges((ti, tj, tw), want_t)
    asymmetric = [(a, b) for (a, b) in want["all"] if xy.ml(a, b) != yx.ml(b, a)]
    assert len(asymmetric) > 0
    forward = dict(zip(zip(i.tolist(), j.tolist()), w.tolist()))
    backward = dict(zip(zip(tj.tolist(), ti.tolist()), tw.tolist()))
    for a, b in asymmetric:
        assert forward.get((a, b)) == (xy(a, b) if xy(a, b) >= 0.121 else None) and backward.get((a, b)) == (yx(b, a) if yx(b, a) >= 0.121 else None)
    assert any(forward.get(p) != backward.get(p) for p in asymmetric)


# ---- the device route on resident data, the cap and the capacity ------------------------------------------------------------------------------
def test_device_route_capacity_and_the_cap(da, mixed_case):
    from dynaalign_amd import device
    seqs, sig, value = mixed_case
    cand = model(sig, 40, 1, 0.5)
    want = nw_model(cand["i"], cand["j"], value, 0.9)
    ds = device.DeviceSequences(*O.pack(seqs))
    device.nw_encode(ds)
    dsig = torch.from_numpy(sig.view(np.int32).copy()).cuda()
    i, j, mt, ln = device.lsh_nw_edges(dsig, ds, N_HASH, 40, 1, 0.9, mh_threshold=0.5)
    torch.cuda.synchronize()
    w = mt.cpu().numpy().astype(np.float64) / ln.cpu().numpy().astype(np.float64)
    same_edges((i.cpu().numpy(), j.cpu().numpy(), w), want)
    assert [value.ml(a, b) for a, b in zip(want["i"], want["j"])] == list(zip(mt.cpu().tolist(), ln.cpu().tolist()))
    # a capacity smaller than the list: the count and the head of the list
    hi, hj, hm, hl = device.lsh_nw_edges(dsig, ds, N_HASH, 40, 1, 0.9, mh_threshold=0.5, capacity=7)
    assert device.nw_lsh_last_route()["edges"] == len(want["i"]) > 7
    assert (hi.cpu().tolist(), hj.cpu().tolist()) == (want["i"][:7], want["j"][:7]) and hm.cpu().tolist() == mt.cpu().tolist()[:7]
    # the cap on the (pair, band) incidences, with the text of the MinHash call
    incidences = model(sig, 40, 1, 0.0)["incidences"]
    for call in (lambda cap: device.lsh_nw_edges(dsig, ds, N_HASH, 40, 1, 0.9, max_candidates=cap),
                 lambda cap: da.similarityNW_lsh_edges(seqs, 4, N_HASH, 40, 1, 0.9, seed=SEED, max_candidates=cap)):
        with pytest.raises(da.DynaAlignError) as e:
            call(incidences - 1)
        with pytest.raises(da.DynaAlignError) as mh:
            da.similarityMH_lsh_edges(seqs, 4, N_HASH, 40, 1, 0.0, seed=SEED, max_candidates=incidences - 1)
        assert e.value.code == UNSUPPORTED and str(e.value) == str(mh.value) and "max_candidates = %d" % (incidences - 1) in str(e.value)
        call(incidences)


def test_device_route_for_two_sets(da, cross_case):
    from dynaalign_amd import device
    x, y, sx, sy = cross_case
    cand = cross_model(sx, sy, 40, 1, 0.0)
    want = nw_model(cand["i"], cand["j"], PairValues(x, y), 0.3)
    dx, dy = device.DeviceSequences(*O.pack(x)), device.DeviceSequences(*O.pack(y))
    device.nw_encode(dx)
    device.nw_encode(dy)
    tx, ty = (torch.from_numpy(s.view(np.int32).copy()).cuda() for s in (sx, sy))
    index = device.lsh_index_build(ty, N_HASH, 40, 1)
    i, j, mt, ln = device.lsh_nw_edges(tx, dx, N_HASH, 40, 1, 0.3, index=index, sig_y=ty, dy=dy)
    w = mt.cpu().numpy().astype(np.float64) / ln.cpu().numpy().astype(np.float64)
    same_edges((i.cpu().numpy(), j.cpu().numpy(), w), want)


def test_clusterbreak_on_the_nw_lsh_graph(da):
    pep = family(1, 6, 20, 300)

    def dense_fn(sub):
        i, j, w = da.nw_lsh_edges_dense(oracle_sig(sub), 12, 4, 0.0, PairValues(sub, sub), 0.5)
        return 0.5, i, j, w
    a = da.clusterbreak(pep, size_max=40, edges_fn=lambda s: da.similarityNW_lsh_edges(s, 4, N_HASH, 12, 4, 0.5, seed=SEED))
    b = da.clusterbreak(pep, size_max=40, edges_fn=dense_fn)
    assert np.array_equal(a["clustered_seq"], b["clustered_seq"]) and a["filtered_seq"] == b["filtered_seq"]
    assert a.calls == b.calls >= 1 and [l["edges"] for l in a.levels] == [l["edges"] for l in b.levels]
