"""GPU tests of the device consensus (clusterconsensus_device / da_cluster_consensus / device.cluster_consensus and the three pieces).
The result is compared EXACTLY with the plain-Python model (tests/nw_align_model.py::consensus) and with the package's own
``clusterconsensus``; the pieces run on synthetic inputs against a few lines of Python: math.fsum for the center, a dict tally for the
vote.  Shapes: the wave boundaries of the reduce (c - 1 = 63, 64, 65), blocks cut in the middle of a member and of a cluster, ops rows
around the 64-op chunks, centers around the strip and window sizes of the kernels."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import nw_align_model as model
from test_gpu_cross import switches

pytestmark = pytest.mark.gpu

SYMBOLS = "ARNDCQEGHILKMFPSTWYVBZX*-"


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


def consensus_rows():
    """the 30 clusters of sizes 1 .. 12 of tests/test_gpu_nw_align.py, by the same recipe"""
    rng = np.random.default_rng(2026)
    rows = []
    for c in range(30):
        root = model.random_seq(rng, 20)
        for _ in range(1 + c % 12):
            rows.append((model.mutate(rng, root, rate=0.2), "c%d" % c))
    order = rng.permutation(len(rows))             # members of a cluster are not adjacent
    return [rows[t] for t in order]


def test_equals_the_model_and_clusterconsensus(da):
    rows = consensus_rows()
    sizes = {}
    for _, cid in rows:
        sizes[cid] = sizes.get(cid, 0) + 1
    assert len(sizes) == 30 and set(sizes.values()) == set(range(1, 13))
    got = da.clusterconsensus_device(rows)
    assert got == model.consensus(rows, aligner=want)
    assert got == da.clusterconsensus(rows)
    assert got == da.clusterconsensus_device(np.array(rows, dtype=object))
    again, centers = da.clusterconsensus_device(rows, return_centers=True)
    assert again == got and [rows[t][1] for t in centers] == [cid for cid, _ in got]
    from dynaalign_amd import device                   # the device call on the pooled table, clusters of one included
    ds, ptr, ids, _ = pooled(da, rows)
    cons, cons_len, _ = device.cluster_consensus(ds, ptr)
    torch.cuda.synchronize()
    assert list(zip(ids, strings(cons, cons_len))) == got


def boundary_rows():
    """tie-heavy clusters at the wave boundaries of the reduce and the chunk boundaries of the vote, the special members, and a handful of
    members at the strip and window sizes of the kernels"""
    rng = np.random.default_rng(77)
    rows = []
    for c in (2, 3, 64, 65, 66, 130):              # c - 1 = 63, 64, 65: one lane short of a wave, a wave, a wave and one
        rows += [(model.random_seq(rng, int(rng.integers(3, 9)), "ACD"), "tie%d" % c) for _ in range(c)]
    rows += [("ACDAC", "same")] * 5                                            # all sums equal: member 0
    rows += [("", "empty-first"), ("ACD", "empty-first"), ("ACD", "empty-first")]
    rows += [("", "empty-center"), ("", "empty-center"), ("", "empty-center")]                      # every sum is 0.0: the center is an empty string
    rows += [("", "all-empty"), ("", "all-empty")]
    rows += [("AC", "gaps-win"), ("", "gaps-win"), ("", "gaps-win")]           # every column is won by '-': the consensus is ""
    for ln in (31, 32, 33, 63, 64, 65, 127):
        root = model.random_seq(rng, ln)
        rows += [(root, "len%d" % ln)] + [(model.mutate(rng, root, rate=0.2, max_len=ln), "len%d" % ln) for _ in range(3)]
    order = rng.permutation(len(rows))
    return [rows[t] for t in order]


@pytest.fixture(scope="module")
def boundary(da):
    rows = boundary_rows()
    return rows, model.consensus(rows, aligner=want)


def test_wave_and_chunk_boundaries_equal_the_model(da, boundary):
    rows, expect = boundary
    assert max(len(s) for s, _ in rows) == 127
    got, centers = da.clusterconsensus_device(rows, return_centers=True)
    assert got == expect
    by_id = dict(got)
    assert by_id["same"] == "ACDAC" and by_id["all-empty"] == "" and by_id["gaps-win"] == "" and by_id["empty-center"] == ""
    ids = [cid for cid, _ in got]
    first = {cid: min(t for t, r in enumerate(rows) if r[1] == cid) for cid in ids}
    for cid in ("same", "empty-center", "all-empty"):                          # equal sums: the first member in input order
        assert centers[ids.index(cid)] == first[cid], cid


def pooled(da, rows):
    """rows -> (DeviceSequences of the members cluster after cluster, cluster_ptr, ids): every cluster, clusters of one included"""
    from dynaalign_amd import device
    ids = list(dict.fromkeys(cid for _, cid in rows))
    seqs, ptr = [], [0]
    for cid in ids:
        seqs += [s for s, c in rows if c == cid]
        ptr.append(len(seqs))
    ds = device.DeviceSequences(*da.pack_sequences(seqs))
    assert int(device.nw_encode(ds).item()) == 0
    return ds, np.array(ptr, np.int64), ids, seqs


def strings(cons, cons_len):
    cons, cons_len = cons.cpu().numpy(), cons_len.cpu().numpy()
    return [bytes(cons[k][:int(cons_len[k])]).decode("latin-1") for k in range(len(cons_len))]


def test_device_call_with_the_smallest_workspace_equals_the_largest(da, boundary):
    """device.cluster_consensus on the pooled table; with blocks of 64 pairs phase 1 cuts inside the members of the clusters of 66 and 130
    (65 and 129 pairs each) and phase 2 takes the clusters of 66 and 130 (65 and 129 rows) in member chunks"""
    from dynaalign_amd import device
    rows, expect = boundary
    ds, ptr, ids, seqs = pooled(da, rows)
    cons, cons_len, center = device.cluster_consensus(ds, ptr)
    torch.cuda.synchronize()
    assert list(zip(ids, strings(cons, cons_len))) == expect
    cen = center.cpu().numpy()
    assert all(ptr[k] <= cen[k] < ptr[k + 1] for k in range(len(ids)))
    small = device.cluster_consensus_workspace_bytes(ptr, ds.max_len, minimal=True)
    assert small < device.cluster_consensus_workspace_bytes(ptr, ds.max_len)
    work = torch.empty(small, dtype=torch.uint8, device="cuda")
    cons2, len2, center2 = device.cluster_consensus(ds, ptr, work=work)
    torch.cuda.synchronize()
    assert torch.equal(len2, cons_len) and torch.equal(center2, center) and strings(cons2, len2) == strings(cons, cons_len)
    with pytest.raises(da.DynaAlignError) as e:
        device.cluster_consensus(ds, ptr, work=work[:small // 2])
    assert e.value.code == 11


def test_blocks_within_the_budget_equal_one_block(da, boundary):
    """DYNAALIGN_BLOCK_BYTES below what blocks of 64 pairs take: the host call then works in exactly such blocks -- phase 1 cuts in the middle
    of members (c - 1 = 65 and 129 terms), phase 2 cuts the clusters of 66 and 130 into member chunks"""
    rows, expect = boundary
    with switches(DYNAALIGN_BLOCK_BYTES=1):
        got, centers = da.clusterconsensus_device(rows, return_centers=True)
    assert got == expect
    assert (got, centers) == da.clusterconsensus_device(rows, return_centers=True)
    with switches(DYNAALIGN_BLOCK_BYTES=3 << 20):                              # a few hundred pairs a block
        assert da.clusterconsensus_device(rows) == expect


def test_long_route_equals_clusterconsensus_with_nw_align_long(da):
    rng = np.random.default_rng(5)
    rows = []
    for k, (ln, c) in enumerate(((128, 3), (129, 4), (513, 3), (1024, 3), (40, 5))):
        root = model.random_seq(rng, ln)
        rows += [(root, "L%d" % k)] + [(model.mutate(rng, root, rate=0.1, max_len=ln), "L%d" % k) for _ in range(c - 1)]
    rows += [(model.random_seq(rng, 700), "alone")]
    order = rng.permutation(len(rows))
    rows = [rows[t] for t in order]
    assert max(len(s) for s, _ in rows) == 1024
    expect = da.clusterconsensus(rows, align_fn=da.nw_align_long)
    assert da.clusterconsensus_device(rows) == expect
    with switches(DYNAALIGN_BLOCK_BYTES=1):
        assert da.clusterconsensus_device(rows) == expect


def test_on_a_clusterbreak_result(da):
    from dynaalign_amd import synth
    seqs = synth.to_strings(*synth.h3n2_like(600, 20))
    res = da.clusterbreak(seqs, thresh_p=0.8, size_max=30, size_min=3, sim_fn=lambda s: da.similarityNW(s), cluster_seed=3)
    labels = list(res["clustered_seq"][:, 1])
    ids = list(dict.fromkeys(labels))
    assert len(ids) > 1
    got, centers = da.clusterconsensus_device(res, return_centers=True)
    assert got == da.clusterconsensus(res)
    assert [c[0] for c in got] == ids and len(centers) == len(ids)
    assert all(labels[t] == cid for t, cid in zip(centers, ids))
    assert da.clusterconsensus_device(res["clustered_seq"]) == got


# ---- the pieces on synthetic inputs --------------------------------------------------------------------------------------------------------
def fsum_centers(terms, ptr):
    """terms[g]: the (matches, length) pairs of pooled member g -> per cluster the pooled index with the largest math.fsum, lowest first"""
    sums = [math.fsum((m / l) if l > 0 else 0.0 for m, l in t) for t in terms]
    return [max(range(ptr[k], ptr[k + 1]), key=lambda g: (sums[g], -g)) for k in range(len(ptr) - 1)]


def run_sums(terms, ptr, cuts=()):
    """center_sums over the concatenated pair results, cut into consecutive calls at `cuts` -> ((members, 2) int64 limbs, centers)"""
    from dynaalign_amd import device
    flat = [p for t in terms for p in t]
    mt = torch.tensor([p[0] for p in flat], dtype=torch.int32, device="cuda")
    ln = torch.tensor([p[1] for p in flat], dtype=torch.int32, device="cuda")
    edges = [0] + list(cuts) + [len(flat)]
    sums = None
    for a, b in zip(edges, edges[1:]):
        sums = device.consensus_center_sums(ln[a:b], mt[a:b], ptr, pair_begin=a, sums=sums)
    center = device.consensus_pick(sums, ptr)
    torch.cuda.synchronize()
    return sums.cpu().numpy(), center.cpu().numpy().tolist()


def exact_limbs(terms):
    out = []
    for t in terms:
        s = sum(int(Fraction(m / l) * 2 ** 63) if l > 0 else 0 for m, l in t)
        out.append([s & (2 ** 64 - 1), s >> 64])
    return np.array(out, np.uint64)


def test_center_sums_round_as_fsum_before_comparing(da):
    thirds, halves = [(1, 3)] * 3, [(1, 2), (1, 4), (1, 4)]
    assert sum(Fraction(m / l) for m, l in thirds) != sum(Fraction(m / l) for m, l in halves)      # the exact sums of the doubles differ ...
    assert math.fsum(m / l for m, l in thirds) == math.fsum(m / l for m, l in halves) == 1.0       # ... and round to the same double
    low = [(1, 5), (0, 7), (2, 9)]
    terms = [thirds, halves, low, low] + [halves, thirds, low, low]
    ptr = [0, 4, 8]
    sums, center = run_sums(terms, ptr)
    assert np.array_equal(sums.view(np.uint64), exact_limbs(terms))
    assert not np.array_equal(sums[0], sums[1])
    assert center == [0, 4] == fsum_centers(terms, ptr)


def test_center_sums_with_empty_pairs_and_cut_blocks(da):
    rng = np.random.default_rng(11)
    ptr, terms = [0], []
    for c in (2, 3, 1, 64, 65, 66, 1, 130, 4):
        for _ in range(c):
            t = []
            for _ in range(c - 1):
                l = int(rng.integers(0, 2049))
                t.append((int(rng.integers(0, min(l, 1024) + 1)), l))
            terms.append(t)
        ptr.append(len(terms))
    terms[ptr[8]] = [(0, 0)] * 3                                               # two empty strings: 0.0
    terms[ptr[8] + 1] = [(0, 0), (1, 3), (0, 0)]
    expect = fsum_centers(terms, ptr)
    sums, center = run_sums(terms, ptr)
    assert np.array_equal(sums.view(np.uint64), exact_limbs(terms)) and center == expect
    total = sum(len(t) for t in terms)
    first130 = sum(len(t) for t in terms[:ptr[7]])
    for cuts in ([first130 + 50], [1, 2, 70, first130 + 129 + 64, total - 1], list(range(64, total, 64))):   # in the middle of members
        sums2, center2 = run_sums(terms, ptr, cuts)
        assert np.array_equal(sums2, sums) and center2 == expect, cuts


def test_pick_takes_the_lowest_index_among_equal_sums_across_lanes(da):
    # 130 equal members: the winner is in lane 0 of the first round; then only member 70 is larger, then members 3 and 67 tie above it
    ptr = [0, 130]
    for bump, expect in (({}, 0), ({70: 1}, 70), ({70: 1, 67: 2, 3: 2}, 3), ({129: 5}, 129)):
        terms = [[(1 + bump.get(g, 0), 7)] + [(1, 3)] * 128 for g in range(130)]
        _, center = run_sums(terms, ptr)
        assert center == [expect] == fsum_centers(terms, ptr), bump


def tally_vote(center, members, ops_rows):
    """clusterconsensus' tally in plain Python: members and ops_rows without the center"""
    tally = [{ch: 1} for ch in center]
    for other, ops in zip(members, ops_rows):
        p = q = 0
        for op in ops:
            if op == "D":
                tally[p][other[q]] = tally[p].get(other[q], 0) + 1
                p += 1
                q += 1
            elif op == "U":
                tally[p]["-"] = tally[p].get("-", 0) + 1
                p += 1
            else:
                q += 1
        assert p == len(center) and q == len(other)
    out = ""
    for p, t in enumerate(tally):
        top = max(t.values())
        tied = [ch for ch in t if t[ch] == top]
        win = center[p] if center[p] in tied else min(tied, key=SYMBOLS.index)
        out += win if win != "-" else ""
    return out


def random_ops(rng, center_len, total):
    """a path of `total` ops over a center of center_len residues -> (ops, member length)"""
    ls = total - center_len
    d = int(rng.integers(0, min(center_len, 127 - ls) + 1)) if ls <= 127 else 0
    ops = ["D"] * d + ["U"] * (center_len - d) + ["L"] * ls
    rng.shuffle(ops)
    return "".join(ops), d + ls


def test_vote_on_hand_made_ops_rows(da):
    from dynaalign_amd import device
    rng = np.random.default_rng(23)
    clusters = []                                   # (center, its place among the members, members, ops rows)
    # leading and trailing L runs, a U run.  Column 0: A 2 (the center's and one member's), R 2, '-' 1 -- the center's A wins the tie; column 1
    # is won by '-' (four U against the center's C); column 2: the center's D 1, C 2, N 2 -- a tie it takes no part in, N comes first
    clusters.append(("ACD", 1, ["WAC", "RCWW", "KKRN", "NK"], ["LDUD", "DUDLL", "LLDUD", "UUDL"]))
    assert tally_vote(*[clusters[0][t] for t in (0, 2, 3)]) == "AN"
    clusters.append(("ACDE", 0, ["", "ACDEW"], ["UUUU", "DDDDL"]))
    cen40 = model.random_seq(rng, 40)
    mem, rows = [], []
    for total in (63, 64, 65, 40, 41, 64, 65):      # rows one short of a chunk of 64 ops, a chunk, a chunk and one
        ops, ml = random_ops(rng, 40, total)
        mem.append(model.random_seq(rng, ml, "ARN" + cen40[:3]))
        rows.append(ops)
    clusters.append((cen40, 3, mem, rows))
    cen127 = model.random_seq(rng, 127, "ARND")
    mem, rows = [], []
    for total in (127, 128, 254, 200, 129, 191, 192, 193):
        ops, ml = random_ops(rng, 127, total)
        mem.append(model.random_seq(rng, ml, "ARND"))
        rows.append(ops)
    clusters.append((cen127, len(mem), mem, rows))
    assert sorted({len(r) for _, _, _, rr in clusters for r in rr} & {63, 64, 65, 127, 128, 254}) == [63, 64, 65, 127, 128, 254]
    seqs, ptr, center, ops_rows = [], [0], [], []
    for cen, at, mem, rows in clusters:
        center.append(len(seqs) + at)
        seqs += mem[:at] + [cen] + mem[at:]
        ptr.append(len(seqs))
        ops_rows += rows
    expect = [tally_vote(cen, mem, rows) for cen, _, mem, rows in clusters]
    assert "" not in expect and any(len(e) < len(c[0]) for e, c in zip(expect, clusters))
    ds = device.DeviceSequences(*da.pack_sequences(seqs))
    assert int(device.nw_encode(ds).item()) == 0
    ld = 254
    ops = np.zeros((len(ops_rows), ld), np.uint8)
    for r, row in enumerate(ops_rows):
        ops[r, :len(row)] = np.frombuffer(row.encode(), np.uint8)
    d_ops = torch.from_numpy(ops).cuda()
    d_center = torch.tensor(center, dtype=torch.int32, device="cuda")
    d_len = torch.tensor([len(r) for r in ops_rows], dtype=torch.int32, device="cuda")
    for length in (d_len, None):                    # without lengths a row ends at its first 0 byte, or at ld_ops
        cons, cons_len = device.consensus_vote(ds, ptr, d_center, d_ops, length)
        torch.cuda.synchronize()
        assert strings(cons, cons_len) == expect, length is None
