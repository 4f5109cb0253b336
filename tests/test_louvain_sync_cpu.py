"""CPU tests of the synchronous Louvain's definition (clusterbreak.louvain_sync_dense, pure numpy) and of the C ABI of its device twin
(da_dev_louvain_workspace_bytes / da_dev_louvain_csr: symbols, workspace size, the refusals made before the device is touched).
The GPU twin -- the device call equals this definition bit for bit -- is tests/test_gpu_louvain_device.py."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
from test_clusterbreak import nx_graph, planted

PLANTED = [(400, 8, .3, .02, 1), (300, 6, .25, .03, 3)]


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    return dynaalign_amd


@pytest.fixture(scope="module")
def graphs(da):
    """name -> (n, ei, ej, ew): the two planted graphs, the thresholded oracle graph and the union kNN graph; built once, never changed"""
    from dynaalign_amd import synth
    from dynaalign_amd.clusterbreak import threshold_edges_dense
    out = {}
    for args in PLANTED:
        out["planted%d" % args[0]] = (args[0],) + planted(*args)
    seqs = synth.to_strings(*synth.h3n2_like(1500, 20))
    rc, M = O.similarity_mh(seqs, 4, 500, O.seeds(12345, 500))
    assert rc == 0
    out["threshold"] = (len(seqs),) + tuple(threshold_edges_dense(M, 0.8)[1:])
    seqs = sorted(set(synth.to_strings(*synth.h3n2_like(3000, 20))))
    rc, M = O.similarity_mh(seqs, 4, 200, O.seeds(12345, 200))
    assert rc == 0
    idx, val = da.knn_dense(M, 5)
    ei, ej, ew = da.knn_graph(idx, val, diag=1.0, mode="union")
    out["knn"] = (len(seqs), np.asarray(ei), np.asarray(ej), np.asarray(ew))
    for g in out.values():
        for a in g[1:]:
            a.setflags(write=False)
    return out


def communities(m):
    return [set(np.nonzero(m == c)[0].tolist()) for c in np.unique(m)]


# ------------------------------------------------------------------ modularity and quality

@pytest.mark.parametrize("name", ["planted400", "planted300"])
@pytest.mark.parametrize("res", [1.05, 0.7])
def test_returned_modularity_is_networkx_modularity_of_the_membership(da, graphs, name, res):
    import networkx as nx
    n, ei, ej, ew = graphs[name]
    m, q, levels, its = da.louvain_sync_dense(n, ei, ej, ew, resolution=res, return_info=True)
    # the quantisation of the weights to 2^-30 is the only difference
    assert abs(nx.community.modularity(nx_graph(n, ei, ej, ew), communities(m), resolution=res) - q) < 1e-6
    assert levels == len(its) and 1 <= levels <= 32 and all(1 <= t <= 64 for t in its)


@pytest.mark.parametrize("name", ["planted400", "planted300", "threshold", "knn"])
def test_quality_against_the_host_louvain(da, graphs, name):
    n, ei, ej, ew = graphs[name]
    host = min(da.louvain(n, ei, ej, ew, seed=s, return_modularity=True)[1] for s in range(4))
    m, q, _, _ = da.louvain_sync_dense(n, ei, ej, ew, return_info=True)
    print("%s: Q = %.6f, smallest host Q over seeds 0..3 = %.6f, ratio %.4f" % (name, q, host, q / host))
    assert q >= 0.97 * host


# ------------------------------------------------------------------ determinism and numbering

def test_result_does_not_depend_on_edge_order_or_orientation(da, graphs):
    n, ei, ej, ew = graphs["planted400"]
    base = da.louvain_sync_dense(n, ei, ej, ew, seed=7, return_info=True)
    rng = np.random.RandomState(2)
    for _ in range(3):
        perm = rng.permutation(len(ei))
        flip = rng.rand(len(ei)) < 0.5
        got = da.louvain_sync_dense(n, np.where(flip, ej, ei)[perm], np.where(flip, ei, ej)[perm], ew[perm], seed=7, return_info=True)
        assert np.array_equal(got[0], base[0]) and got[1:] == base[1:]


def test_ids_start_at_one_in_order_of_first_appearance(da, graphs):
    for name in ("planted300", "knn"):
        n, ei, ej, ew = graphs[name]
        m = da.louvain_sync_dense(n, ei, ej, ew)
        assert m.dtype == np.int32 and m.shape == (n,)
        _, first = np.unique(m, return_index=True)
        assert m[0] == 1 and np.array_equal(m[np.sort(first)], np.arange(1, len(first) + 1))
    n = 90
    ei, ej, ew = planted(n, 3, 0.7, 0.01, 0)
    assert da.louvain_sync_dense(n, ei, ej, ew).tolist() == [1] * 30 + [2] * 30 + [3] * 30


def test_it_is_a_cluster_fn(da):
    """netcluster / clusterbreak call cluster_fn(n, i, j, w, seed=, weights=) and take a numeric vector of n ids"""
    n = 90
    ei, ej, ew = planted(n, 3, 0.7, 0.01, 0)
    M = np.zeros((n, n))
    M[ei, ej] = ew
    assert da.netcluster(M, cluster_func=da.louvain_sync_dense).tolist() == [1] * 30 + [2] * 30 + [3] * 30


# ------------------------------------------------------------------ edge cases

def test_edge_cases(da):
    f = da.louvain_sync_dense
    assert f(0, [], [], []).tolist() == []
    m, q, levels, its = f(4, [], [], [], return_info=True)                       # no edges: everyone alone, nothing to iterate
    assert (m.tolist(), q, levels, its) == ([1, 2, 3, 4], 0.0, 0, [])
    m, q, levels, its = f(3, [0, 1, 2], [0, 1, 2], [1.0, 1.0, 1.0], return_info=True)   # loops only
    assert m.tolist() == [1, 2, 3] and (levels, its) == (1, [1])
    assert q == 1.0 - 1.05 * (3 * 4.0 / 36.0)
    m, q, levels, its = f(1, [0], [0], [1.0], return_info=True)
    assert m.tolist() == [1] and (levels, its) == (1, [1]) and q == 1.0 - 1.05
    assert f(1, [], [], []).tolist() == [1]
    assert f(2, [0], [1], [0.5]).tolist() == [1, 1]                              # two vertices and one edge
    assert f(4, [2, 0], [3, 1], [1.0, 1.0]).tolist() == [1, 1, 2, 2]
    assert f(5, [2, 0], [3, 1], [1.0, 1.0]).tolist() == [1, 1, 2, 2, 3]          # an isolated vertex without a loop
    # weights=False: the heavy bridge no longer decides
    ei, ej = np.array([0, 0, 1, 3, 3, 4, 2], np.int32), np.array([1, 2, 2, 4, 5, 5, 3], np.int32)
    ew = np.array([1, 1, 1, 1, 1, 1, 50.0])
    assert f(6, ei, ej, ew, weights=False).tolist() == [1, 1, 1, 2, 2, 2]
    assert f(6, ei, ej, ew).tolist() != [1, 1, 1, 2, 2, 2]
    assert np.array_equal(f(6, ei, ej, ew, weights=False), f(6, ei, ej, np.ones(7)))


def test_refusals(da):
    f = da.louvain_sync_dense
    with pytest.raises(ValueError):
        f(3, [0], [1], [float("nan")])
    with pytest.raises(ValueError):
        f(3, [0], [1], [float("inf")])
    with pytest.raises(ValueError):
        f(3, [0], [1], [-0.5])
    with pytest.raises(ValueError):
        f(3, [0], [5], [1.0])
    with pytest.raises(ValueError):
        f(3, [-1], [1], [1.0])
    with pytest.raises(ValueError):
        f(3, [0, 1], [1], [1.0])
    with pytest.raises(ValueError):
        f(3, [0, 1], [1, 2], [2.0 ** 31, 2.0 ** 31])                             # 2m could reach 2^62


def test_canonical_csr_of_louvain_device(da):
    """what louvain_device uploads: repeated edges and too many distinct weights are refused before any device call"""
    from dynaalign_amd.clusterbreak import canonical_csr
    ptr, adj, codes, loops, values = canonical_csr(4, [3, 0, 1], [2, 1, 1], [0.5, 0.25, 1.0])
    assert ptr.tolist() == [0, 1, 2, 3, 4] and adj.tolist() == [1, 0, 3, 2]
    assert values.tolist() == [0.25, 0.5, 1.0] and codes.tolist() == [0, 0, 1, 1] and loops.tolist() == [0xFFFF, 2, 0xFFFF, 0xFFFF]
    with pytest.raises(ValueError):
        canonical_csr(3, [0, 1], [1, 0], [1.0, 1.0])
    for bad in (float("nan"), float("inf"), -0.5):                              # refused like louvain_sync_dense refuses them
        with pytest.raises(ValueError):
            canonical_csr(3, [0, 1], [1, 2], [1.0, bad])
    with pytest.raises(ValueError):
        canonical_csr(3, [0], [3], [1.0])
    with pytest.raises(ValueError):
        canonical_csr(70000, np.arange(66000), np.arange(66000) + 1, np.arange(66000) + 1.0)
    with pytest.raises(ValueError):
        da.clusterbreak(["AAAA"] * 4, louvain="device")                          # needs a session
    with pytest.raises(ValueError):
        da.clusterbreak(["AAAA"] * 4, louvain="gpu")


def test_device_mode_refuses_the_switch_that_turns_the_csr_path_off(da, monkeypatch):
    class FakeSession:
        n = 4
    monkeypatch.setenv("DYNAALIGN_CLUSTERBREAK_NO_CSR", "1")
    with pytest.raises(ValueError, match="DYNAALIGN_CLUSTERBREAK_NO_CSR"):
        da.clusterbreak(["AAAA"] * 4, session=FakeSession(), louvain="device")


# ------------------------------------------------------------------ C ABI

def test_abi_symbols_and_workspace_size(da):
    from dynaalign_amd import _capi
    lib = _capi.load()
    for name in ("da_dev_louvain_workspace_bytes", "da_dev_louvain_csr"):
        assert hasattr(lib, name) and name in _capi.SIGNATURES and name in _capi.header_symbols()
    assert hasattr(da, "louvain_sync_dense") and hasattr(da, "louvain_device")
    w = lib.da_dev_louvain_workspace_bytes
    assert w(0, 0) > 0 and w(-5, -5) > 0
    ns, zs = [0, 1, 63, 64, 1000, 4096, 4097, 100000], [0, 1, 64, 65, 3072, 3073, 10 ** 5, 10 ** 7]
    for z in zs:
        sizes = [w(n, z) for n in ns]
        assert sizes == sorted(sizes), (z, sizes)
    for n in ns:
        sizes = [w(n, z) for z in zs]
        assert sizes == sorted(sizes), (n, sizes)
    assert w(1000, 10 ** 6) >= 10 ** 6 * 12                                      # the coarse graph alone
    # beyond what the call accepts the size is that of the limits (the call refuses such a graph), never a wrapped item count
    assert w(1 << 40, 1 << 40) == w((1 << 31) - 16, (1 << 31) - 256) >= w(100000, 10 ** 7)


def test_abi_refusals_before_the_device_is_touched(da):
    from dynaalign_amd import _capi
    lib = _capi.load()
    BAD = _capi.DA_ERR_BAD_ARG
    q, lv, its = ctypes.c_double(7.0), ctypes.c_int32(7), (ctypes.c_int32 * 32)()
    values = np.array([0.5, 1.0])
    fake = 1 << 20                                                               # a non-NULL, 256-aligned address that is never dereferenced
    need = lib.da_dev_louvain_workspace_bytes(5, 0)

    def call(n=5, ptr=fake, adj=fake, codes=fake, loops=None, vals=values.ctypes.data, nv=2, res=1.05, work=fake, wb=need, member=fake):
        return lib.da_dev_louvain_csr(n, ptr, adj, codes, loops, vals, nv, res, 0, work, wb, member, ctypes.byref(q), ctypes.byref(lv), its, None)
    assert call(n=-1) == BAD
    assert call(n=1 << 40) == _capi.DA_ERR_UNSUPPORTED
    assert call(ptr=None) == BAD
    assert call(work=None) == BAD
    assert call(member=None) == BAD
    assert call(vals=None) == BAD
    assert call(nv=-1) == BAD and call(nv=70000) == BAD
    assert call(wb=need - 1) == BAD and call(wb=0) == BAD
    assert call(work=fake + 8) == BAD                                            # not 256-byte aligned
    assert call(res=float("nan")) == BAD
    assert call(n=0, ptr=None, work=None, member=None, wb=0) == _capi.DA_OK      # nothing to cluster
    assert (q.value, lv.value) == (0.0, 0)
