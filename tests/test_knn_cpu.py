"""CPU tests of the one-set nearest-neighbour forms: knn_dense and knn_graph (the definitions in numpy) against brute-force constructions,
and clusterbreak on a kNN graph handed over as edges_fn.  No device is needed: the similarity matrices come from the CPU oracle."""
import numpy as np
import pytest

import oracle_lib as O

SEED = 12345


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    return dynaalign_amd


def brute_lists(S, top):
    n = S.shape[0]
    idx = np.zeros((n, top), np.int32)
    val = np.zeros((n, top), np.float64)
    for i in range(n):
        cand = [j for j in range(n) if j != i]
        cand.sort(key=lambda j: (-S[i, j], j))
        for t in range(top):
            idx[i, t], val[i, t] = cand[t], S[i, cand[t]]
    return idx, val


def brute_graph(idx, val, diag, mode):
    n = idx.shape[0]
    live = {}
    for i in range(n):
        for j, v in zip(idx[i], val[i]):
            if v > 0:
                live[(i, int(j))] = v
    out = {}
    for (i, j), v in live.items():
        back = (j, i) in live
        if mode == "union" or back:
            a, b = min(i, j), max(i, j)
            out[(a, b)] = live[(a, b)] if (a, b) in live else live[(b, a)]      # the smaller row's entry when it has one
    if diag is not None:
        d = np.broadcast_to(np.asarray(diag, np.float64), (n,))
        for i in range(n):
            out[(i, i)] = d[i]
    keys = sorted(out)
    return (np.array([a for a, _ in keys], np.int32), np.array([b for _, b in keys], np.int32), np.array([out[q] for q in keys], np.float64))


def symmetric(rng, n, levels, zero_share):
    A = rng.randint(0, levels, (n, n)).astype(np.float64) / max(levels - 1, 1)
    A[rng.rand(n, n) < zero_share] = 0.0
    S = np.triu(A, 1)
    S = S + S.T
    np.fill_diagonal(S, 1.0)
    return S


@pytest.mark.parametrize("n,levels,zero_share", [(2, 2, 0.0), (3, 2, 0.5), (7, 3, 0.3), (20, 4, 0.6), (33, 50, 0.0), (12, 1, 0.0), (9, 3, 1.0)])
def test_knn_dense_against_a_brute_force_loop(da, n, levels, zero_share):
    S = symmetric(np.random.RandomState(n), n, levels, zero_share)
    for top in sorted({1, min(3, n - 1), n - 1}):
        idx, val = da.knn_dense(S, top)
        want_idx, want_val = brute_lists(S, top)
        assert idx.dtype == np.int32 and val.dtype == np.float64 and idx.shape == (n, top)
        assert np.array_equal(idx, want_idx) and np.array_equal(val.view(np.uint64), want_val.view(np.uint64))
        assert not (idx == np.arange(n)[:, None]).any()                        # never the row itself
    M = S.copy()
    np.fill_diagonal(M, -np.inf)
    assert np.array_equal(da.knn_dense(S, n - 1)[0], np.argsort(-M, axis=1, kind="stable")[:, :n - 1])


def test_knn_dense_refuses_bad_arguments(da):
    S = symmetric(np.random.RandomState(1), 4, 3, 0.0)
    for top in (0, 4, -1):
        with pytest.raises(ValueError):
            da.knn_dense(S, top)
    with pytest.raises(ValueError):
        da.knn_dense(np.ones((1, 1)), 1)
    with pytest.raises(ValueError):
        da.knn_dense(np.ones((2, 3)), 1)


@pytest.mark.parametrize("mode", ["union", "mutual"])
def test_knn_graph_against_a_set_construction(da, mode):
    for n, levels, zero_share, top in [(5, 3, 0.0, 2), (16, 4, 0.5, 3), (30, 6, 0.2, 5), (30, 2, 0.8, 29), (8, 3, 1.0, 2)]:
        S = symmetric(np.random.RandomState(100 + n + top), n, levels, zero_share)
        idx, val = da.knn_dense(S, top)
        for diag in (None, np.diag(S).copy(), 1.0):
            got = da.knn_graph(idx, val, diag, mode)
            want = brute_graph(idx, val, diag, mode)
            assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.float64
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), (n, top, diag is None)
            assert (got[0] <= got[1]).all() and (got[2] > 0).all()
            assert np.array_equal(np.lexsort((got[1], got[0])), np.arange(len(got[0])))       # sorted by (i, j)
            assert ((got[0] == got[1]).sum() == (0 if diag is None else n))


def test_knn_graph_asymmetric_lists_zeros_and_diagonal(da):
    # 0 is everybody's best neighbour, but 0 lists only 1: (2 -> 0) and (3 -> 0) are one-sided
    idx = np.array([[1], [0], [0], [0]], np.int32)
    val = np.array([[0.9], [0.9], [0.5], [0.25]])
    i, j, w = da.knn_graph(idx, val, None, "union")
    assert (i.tolist(), j.tolist(), w.tolist()) == ([0, 0, 0], [1, 2, 3], [0.9, 0.5, 0.25])
    i, j, w = da.knn_graph(idx, val, None, "mutual")
    assert (i.tolist(), j.tolist(), w.tolist()) == ([0], [1], [0.9])
    idx = np.array([[1, 2], [0, 2], [0, 1]], np.int32)
    val = np.array([[0.5, 0.0], [0.5, 0.0], [0.0, 0.0]])                       # zero-valued entries are no edges, from either side
    for mode in ("union", "mutual"):
        i, j, w = da.knn_graph(idx, val, None, mode)
        assert (i.tolist(), j.tolist(), w.tolist()) == ([0], [1], [0.5])
        i, j, w = da.knn_graph(idx, val, [1.0, 0.75, 1.0], mode)
        assert (i.tolist(), j.tolist(), w.tolist()) == ([0, 0, 1, 2], [0, 1, 1, 2], [1.0, 0.5, 0.75, 1.0])
    with pytest.raises(ValueError):
        da.knn_graph(idx, val, None, "both")


def peptides(rng, n):
    base = ["".join("ACDEFGHIKLMNPQRSTVWY"[i] for i in rng.randint(0, 20, 14)) for _ in range(8)]
    out = []
    for t in range(n):
        s = list(base[t % len(base)])
        s[rng.randint(0, len(s))] = "ACDEFGHIKLMNPQRSTVWY"[rng.randint(0, 20)]
        out.append("".join(s) + "ACDEFGHIKLMNPQRSTVWY"[t % 20] * (t // 20 % 3))
    return out


def test_clusterbreak_on_a_knn_graph_through_edges_fn(da):
    seqs = peptides(np.random.RandomState(5), 120)
    k, n_hash, top = 3, 64, 6
    seeds = O.seeds(SEED, n_hash)
    calls = []

    def edges(shuffle):
        def fn(sub):
            rc, S = O.similarity_mh(sub, k, n_hash, seeds)
            assert rc == 0
            t = min(top, len(sub) - 1)
            idx, val = da.knn_dense(S, t)
            i, j, w = da.knn_graph(idx, val, np.diag(S).copy(), "union")
            calls.append(len(i))
            assert len(i) <= len(sub) * (t + 1)                                # at most n * top edges + the diagonal
            if shuffle:
                p = np.random.RandomState(len(sub)).permutation(len(i))
                i, j, w = i[p], j[p], w[p]
            off = w[i != j]
            return (off.min() if len(off) else float("nan")), i, j, w
        return fn
    a = da.clusterbreak(seqs, size_max=30, size_min=2, edges_fn=edges(False), cluster_seed=3)
    b = da.clusterbreak(seqs, size_max=30, size_min=2, edges_fn=edges(True), cluster_seed=3)
    assert len(a["clustered_seq"]) + len(a["filtered_seq"]) == len(seqs) and len(a["clustered_seq"]) > 0
    assert len(set(a["clustered_seq"][:, 1])) > 1
    assert np.array_equal(a["clustered_seq"], b["clustered_seq"]) and a["filtered_seq"] == b["filtered_seq"]
    assert calls


def test_clusterbreak_knn_needs_a_session(da):
    with pytest.raises(ValueError) as e:
        da.clusterbreak(["ACDEFG", "ACDEFH", "ACDEFK", "ACDEFL"], knn=5)
    assert "edges_fn=lambda s: similarityMH_knn_edges(s" in str(e.value)
    import inspect
    sig = inspect.signature(da.clusterbreak)
    assert sig.parameters["knn"].default is None and sig.parameters["knn_mode"].default == "union"
    assert sig.parameters["knn"].kind is inspect.Parameter.KEYWORD_ONLY
