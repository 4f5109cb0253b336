"""GPU tests of the matrix-free statistics -- similarityMH_stats, similarityNW_stats, similarityNW_stats_long, MinHashSession.stats -- end to end
against the CPU oracle's dense matrix R and numpy:
    U = R[np.triu_indices(n, 1)]; np.median(U), U.min(), U.max(), math.fsum(U) / U.size;
    the reference's pair: tuple(np.argwhere(R.T == v)[0][::-1]); the *_upper pair: np.argwhere(np.triu(R == v, 1))[0].
All comparisons are exact (doubles as uint64 bit patterns, positions as integers) except the mean: 2 ** -40 relative, the bound derived in
test_stats_cpu.py.  Each device result is also held against compute_similarity_stats of the package's own dense matrix."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from test_gpu_cross import switches
from test_gpu_nw_edges_long import fit, mutate, rand_seq, square_input, square_oracle
from test_stats_cpu import assert_stats

pytestmark = pytest.mark.gpu

SEED = 12345


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    from dynaalign_amd import _capi
    assert _capi.load().da_device_count() > 0
    return dynaalign_amd


def same(a, b):
    """two SimilarityStats equal field for field, the doubles bit for bit"""
    return tuple(a[4:]) == tuple(b[4:]) and np.array_equal(np.array(a[:4]).view(np.uint64), np.array(b[:4]).view(np.uint64))


# ---- MinHash ----------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def mh_input(n, duplicates):
    """n h3n2-like 20-mers, all different -- or with a few exact copies planted, none of them involving sequence 0"""
    from dynaalign_amd import synth
    res, off = synth.h3n2_like(4 * n, 20)
    seqs = list(dict.fromkeys(synth.to_strings(res, off)))[:n]
    assert len(seqs) == n
    if duplicates:
        for src, dst in ((17, 40), (17, 41), (n // 2, n - 3)):
            seqs[dst] = seqs[src]
    return tuple(seqs)


@functools.lru_cache(maxsize=None)
def mh_oracle(seqs, k, n_hash):
    from dynaalign_amd import hash_family_seeds
    rc, R = O.similarity_mh(list(seqs), k, n_hash, hash_family_seeds(SEED, n_hash))
    assert rc == 0
    R.setflags(write=False)
    return R


@pytest.mark.parametrize("n", [2, 3])
def test_mh_smallest_inputs(da, n):
    seqs = ("ACDEFGHIKLMNPQRSTVWY", "ACDEFGHIKLMNPQRSTVWA", "YWVTSRQPNMLKIHGFEDCA")[:n]
    got = da.similarityMH_stats(list(seqs), 4, 50, seed=SEED)
    assert_stats(got, mh_oracle(seqs, 4, 50), n)
    assert same(got, da.compute_similarity_stats(da.similarityMH(list(seqs), 4, 50, seed=SEED)))


@pytest.mark.parametrize("n_hash", [50, 500])
def test_mh_without_duplicates(da, n_hash):
    seqs = mh_input(300, False)
    R = mh_oracle(seqs, 4, n_hash)
    assert R[np.triu_indices(300, 1)].max() < 1.0                          # the condition: no two signatures are equal
    got = da.similarityMH_stats(list(seqs), 4, n_hash, seed=SEED)
    assert_stats(got, R, n_hash)
    assert got.most_similar_pair[0] > got.most_similar_pair[1] and got.most_similar_upper == got.most_similar_pair[::-1]
    assert same(got, da.compute_similarity_stats(da.similarityMH(list(seqs), 4, n_hash, seed=SEED)))


def test_mh_with_duplicates_the_reference_lands_on_the_diagonal(da):
    seqs = mh_input(300, True)
    R = mh_oracle(seqs, 4, 50)
    got = da.similarityMH_stats(list(seqs), 4, 50, seed=SEED)
    assert_stats(got, R)
    assert got.max_similarity == 1.0 and got.most_similar_pair == (0, 0) and got.most_similar_upper == (17, 40)
    assert same(got, da.compute_similarity_stats(da.similarityMH(list(seqs), 4, 50, seed=SEED)))


def test_mh_1500_sequences(da):
    seqs = mh_input(1500, True)
    assert_stats(da.similarityMH_stats(list(seqs), 4, 50, seed=SEED), mh_oracle(seqs, 4, 50))


def test_session_stats_of_a_subset(da):
    from dynaalign_amd.session import MinHashSession
    seqs = mh_input(300, True)
    s = MinHashSession(list(seqs), 4, 50, seed=SEED, reserve=False)
    rng = np.random.RandomState(8)
    for idx in (None, np.sort(rng.choice(300, 120, replace=False)), rng.permutation(300)[:77], np.array([40, 17])):
        sub = list(seqs) if idx is None else [seqs[t] for t in idx]
        got = s.stats(idx)
        assert same(got, da.similarityMH_stats(sub, 4, 50, seed=SEED)), idx
        assert_stats(got, mh_oracle(tuple(sub), 4, 50))
    with pytest.raises(da.DynaAlignError) as ei:
        s.stats(np.array([5]))
    assert ei.value.code == 11 and "need >= 2 sequences" in str(ei.value)


# ---- NW -----------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def nw_short_input():
    """150 sequences of 1 .. 127 residues: unrelated strings of every kind of length, families of near-copies (one substitution, one residue
    dropped), exact copies, single residues and a few with X -- the values tie across (matches, length): 1/2 from 'A' against 'AC' and from longer pairs"""
    rng = np.random.RandomState(606)
    seqs = ["A", "C", "AC", "CA", "ACAC", "W" * 127, "W" * 126 + "A", "XX", "AXA", "XAX", "AXXA"]      # X against X scores -1: see the free-gap test
    parents = [rand_seq(rng, length) for length in (127, 90, 41, 12)]
    for p in parents:
        seqs.append(p)
        for _ in range(6):
            seqs.append(fit(rng, mutate(rng, p, 0.04), min(127, len(p) + int(rng.randint(0, 3)))))
        seqs.append(p)                                                    # an exact copy
    while len(seqs) < 150:
        seqs.append(rand_seq(rng, int(rng.randint(1, 128))))
    order = rng.permutation(len(seqs))
    seqs = [seqs[t] for t in order]
    assert min(map(len, seqs)) == 1 and max(map(len, seqs)) == 127
    return tuple(seqs)


@pytest.mark.parametrize("matrix,go,ge", [("BLOSUM62", 10, 4), ("BLOSUM45", 0, 0)])
def test_nw_short_against_the_oracle(da, matrix, go, ge):
    seqs = nw_short_input()
    R = square_oracle(seqs, matrix, go, ge)[0]
    got = da.similarityNW_stats(list(seqs), matrix, go, ge)
    assert_stats(got, R, (matrix, go, ge))
    assert same(got, da.compute_similarity_stats(da.similarityNW(list(seqs), matrix, go, ge)))
    assert same(got, da.similarityNW_stats_long(list(seqs), matrix, go, ge))       # the two calls agree field for field


def test_nw_free_gaps_give_a_diagonal_that_is_not_one(da):
    """gapOpen = gapExt = 0: the alignment of a sequence with itself may prefer gaps to a residue whose self score is not the best on offer,
    and the diagonal is what the DP says, not 1.0"""
    seqs = nw_short_input()
    R = square_oracle(seqs, "BLOSUM62", 0, 0)[0]
    diag = R.diagonal()
    assert (diag != 1.0).sum() == 4 and diag.min() == 1.0 / 3.0                 # 'XX' with itself: X-, -X, X- ... one match in three columns
    got = da.similarityNW_stats(list(seqs), "BLOSUM62", 0, 0)
    assert_stats(got, R)
    assert same(got, da.similarityNW_stats_long(list(seqs), "BLOSUM62", 0, 0))


def test_nw_long_in_one_block_and_in_blocks_of_eight_rows(da):
    seqs = square_input()                                                 # 44 sequences of 1 .. 300 residues
    R = square_oracle(seqs, "BLOSUM62", 10, 4)[0]
    whole = da.similarityNW_stats_long(list(seqs))
    with switches(DYNAALIGN_BLOCK_BYTES=1500):                            # 44 columns of 4 bytes: 8 rows a block, 6 blocks
        blocked = da.similarityNW_stats_long(list(seqs))
    assert_stats(whole, R, "one block")
    assert_stats(blocked, R, "8-row blocks")
    assert same(whole, blocked)
    assert same(whole, da.compute_similarity_stats(da.similarityNW(list(seqs))))
    with pytest.raises(da.DynaAlignError) as ei:
        da.similarityNW_stats(list(seqs))
    assert ei.value.code == 10 and "127" in str(ei.value)
