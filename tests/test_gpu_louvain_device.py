"""The device Louvain (da_dev_louvain_csr, csrc/louvain_kernels.hip) against its definition, clusterbreak.louvain_sync_dense:
membership, modularity (==), levels and iterations per level must be EQUAL -- integer sums and one fixed gain expression leave no
room for a tolerance.  Graphs are chosen so that every decide kernel runs: the wave bin (rows of <= 64 entries), the LDS table in both
its forms (open addressing on a level of more than 4096 vertices, indexed by community below), long rows that try the LDS table first, the
table in the workspace (two hubs of class 0 with more neighbours than the LDS table has slots: test_two_hubs_overflow_into_the_workspace_table
says why they must fall through), and coarse levels with int64 weights."""

import numpy as np
import pytest

from test_clusterbreak import planted

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    from dynaalign_amd import _capi
    assert _capi.load().da_device_count() > 0
    return dynaalign_amd


@pytest.fixture(scope="module")
def h3n2(da):
    from dynaalign_amd import synth
    from dynaalign_amd.session import MinHashSession
    seqs = synth.to_strings(*synth.h3n2_like(3000, 20))
    return seqs, MinHashSession(seqs, 4, 200, seed=12345)


def upload(ptr, adj, codes, loops):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(ptr, np.int64)).cuda(), torch.from_numpy(np.ascontiguousarray(adj, np.int32)).cuda(),
            torch.from_numpy(np.ascontiguousarray(codes, np.uint16).view(np.int16)).cuda(),
            torch.from_numpy(np.ascontiguousarray(loops, np.uint16).view(np.int16)).cuda())


def host_csr(t):
    ptr, adj, codes, loops = t
    return ptr.cpu().numpy(), adj.cpu().numpy(), codes.cpu().numpy().view(np.uint16), loops.cpu().numpy().view(np.uint16)


def assert_equals_model(da, dev_csr, values, resolution=1.05, seed=0, weights=True):
    """device.louvain_csr on the device CSR == louvain_sync_dense on the same graph as an edge list"""
    from dynaalign_amd import device
    from dynaalign_amd.clusterbreak import _csr_to_edges
    ptr, adj, codes, loops = host_csr(dev_csr)
    n = len(ptr) - 1
    ei, ej, ew = _csr_to_edges(ptr, adj, codes, loops, np.asarray(values, np.float64))
    want = da.louvain_sync_dense(n, ei, ej, ew, resolution=resolution, seed=seed, weights=weights, return_info=True)
    got = device.louvain_csr(*dev_csr, values, resolution=resolution, seed=seed, weights=weights)
    print("n=%d nnz=%d res=%g seed=%d: model Q=%r levels=%d iterations=%s | device Q=%r levels=%d iterations=%s, %d communities"
          % (n, len(adj), resolution, seed, want[1], want[2], want[3], got[1], got[2], got[3], int(got[0].max()) if n else 0))
    assert got[2] == want[2] and got[3] == want[3]
    assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0])
    assert got[1] == want[1]
    return got


def edge_list_csr(da, n, ei, ej, ew):
    from dynaalign_amd.clusterbreak import canonical_csr
    ptr, adj, codes, loops, values = canonical_csr(n, ei, ej, ew)
    return upload(ptr, adj, codes, loops), values


def hub_graph(n):
    """vertices 0 .. n-3 in cliques (the first 400 in cliques of 100, the rest in cliques of 20) at code 100, a half hub n-2 joined to the
    first 2500 vertices and a hub n-1 joined to every vertex, both at code 1: rows of 21, 101, 2500 and n-1 entries"""
    group = np.where(np.arange(n - 2) < 400, np.arange(n - 2) // 100, 4 + (np.arange(n - 2) - 400) // 20)
    a, b = np.nonzero(np.triu(group[:, None] == group[None, :], 1))
    ei = np.concatenate([a, np.arange(2500), np.arange(n - 1)])
    ej = np.concatenate([b, np.full(2500, n - 2), np.full(n - 1, n - 1)])
    code = np.concatenate([np.full(len(a), 100), np.full(2500 + n - 1, 1)])
    lo, hi = np.minimum(ei, ej), np.maximum(ei, ej)
    aa, bb, cc = np.concatenate([lo, hi]), np.concatenate([hi, lo]), np.concatenate([code, code])
    o = np.lexsort((bb, aa))
    ptr = np.zeros(n + 1, np.int64)
    np.add.at(ptr, aa + 1, 1)
    return np.cumsum(ptr), bb[o].astype(np.int32), cc[o].astype(np.uint16), np.full(n, 0xFFFF, np.uint16)


# ------------------------------------------------------------------ equality with the model

@pytest.mark.parametrize("args", [(400, 8, .3, .02, 1), (1000, 10, .1, .02, 5)])
@pytest.mark.parametrize("res,seed", [(1.05, 0), (0.7, 7)])
def test_planted_graphs(da, args, res, seed):
    csr, values = edge_list_csr(da, args[0], *planted(*args))
    got = assert_equals_model(da, csr, values, res, seed)
    assert got[2] >= 2                                             # coarse levels ran


def test_thresholded_session_graph_the_lds_bin(da, h3n2):
    from dynaalign_amd import device
    seqs, sess = h3n2
    thr, n_edges, ptr, adj, codes, loops, values = sess.edges_csr(None, .8, on_device=True)
    assert ptr.is_cuda and adj.is_cuda and codes.is_cuda and loops.is_cuda
    deg = np.diff(ptr.cpu().numpy())
    assert deg.max() > device.LOUVAIN_WAVE_MAX                      # rows for the workgroup kernel
    host = sess.edges_csr(None, .8)                                 # on_device=False: exactly what it returned before
    assert host[0] == thr and host[1] == n_edges
    for a, b in zip(host_csr((ptr, adj, codes, loops)), host[2:6]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert_equals_model(da, (ptr, adj, codes, loops), values)
    assert_equals_model(da, (ptr, adj, codes, loops), values, 0.7, 7)


def test_knn_session_graph_the_wave_bin(da, h3n2):
    from dynaalign_amd import device
    seqs, sess = h3n2
    thr, n_edges, ptr, adj, codes, loops, values = sess.knn_csr_device(top=5)
    host = sess.knn_csr(top=5)
    assert (host[0] == thr or (np.isnan(thr) and np.isnan(host[0]))) and host[1] == n_edges
    for a, b in zip(host_csr((ptr, adj, codes, loops)), host[2:6]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert np.diff(host[2]).min() <= device.LOUVAIN_WAVE_MAX
    assert_equals_model(da, (ptr, adj, codes, loops), values)
    assert_equals_model(da, (ptr, adj, codes, loops), values, 0.7, 7)
    assert_equals_model(da, (ptr, adj, codes, loops), values, weights=False)
    # the LSH form of the same graph keeps its CSR on the device the same way
    dev = sess.lsh_knn_csr_device(20, 5, top=5)
    host = sess.lsh_knn_csr(20, 5, top=5)
    assert (host[0] == dev[0] or (np.isnan(dev[0]) and np.isnan(host[0]))) and host[1] == dev[1]
    for a, b in zip(host_csr(dev[2:6]), host[2:6]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert_equals_model(da, dev[2:6], dev[6])


@pytest.mark.parametrize("extra", ["lds", "direct"])
def test_hub_graph_every_bin(da, extra):
    """n = limit + about 200: above LOUVAIN_DIRECT_MAX the hub row (n - 1 entries > LOUVAIN_LDS_MAX) is a long row -- it tries the LDS table
    first, and here its communities fit (the workspace table is test_two_hubs_overflow_into_the_workspace_table's) -- and the rows of 101 and
    2500 entries take the open-addressing LDS table; at LOUVAIN_LDS_MAX + 200 the level is indexed by community"""
    from dynaalign_amd import device
    n = (device.LOUVAIN_DIRECT_MAX if extra == "lds" else device.LOUVAIN_LDS_MAX) + 205
    assert n - 1 > device.LOUVAIN_LDS_MAX
    csr = upload(*hub_graph(n))
    values = np.arange(201, dtype=np.float64) / 200
    assert_equals_model(da, csr, values)
    assert_equals_model(da, csr, values, 0.7, 7)


def vertex_class(v, seed, level=0):
    return (((v * 2654435761 + seed * 40503 + level) & (2 ** 64 - 1)) >> 7) & 7


def two_hub_graph(n, hubs):
    """the vertices other than `hubs` in cliques of 20 at code 100; every hub joined to every other vertex (the other hub too) at code 1"""
    rest = np.setdiff1d(np.arange(n), hubs)
    group = np.arange(len(rest)) // 20
    a, b = np.nonzero(np.triu(group[:, None] == group[None, :], 1))
    ei, ej, code = [rest[a]], [rest[b]], [np.full(len(a), 100)]
    for t, h in enumerate(hubs):
        other = np.setdiff1d(np.arange(n), hubs[:t + 1])            # a hub pair is listed once
        ei.append(np.full(len(other), h)); ej.append(other); code.append(np.full(len(other), 1))
    ei, ej, code = np.concatenate(ei), np.concatenate(ej), np.concatenate(code)
    aa, bb, cc = np.concatenate([ei, ej]), np.concatenate([ej, ei]), np.concatenate([code, code])
    o = np.lexsort((bb, aa))
    ptr = np.zeros(n + 1, np.int64)
    np.add.at(ptr, aa + 1, 1)
    return np.cumsum(ptr), bb[o].astype(np.int32), cc[o].astype(np.uint16), np.full(n, 0xFFFF, np.uint16)


@pytest.mark.parametrize("res,seed", [(1.05, 0), (0.7, 7)])
def test_two_hubs_overflow_into_the_workspace_table(da, res, seed):
    """The workspace table (k_lv_decide_table<., 2>) is reached only by a long row whose neighbouring communities do not fit the LDS table.
    Here that is certain, whatever the order in which lanes arrive: vertices 303 and 1327 have class 0 at level 0 for seed 0 and for seed 7,
    so they decide in the first sub-round of the first iteration, from the snapshot in which every vertex is its own community; each has
    n - 1 = 4499 neighbours, hence 4499 distinct keys for LOUVAIN_LDS_SLOTS = 4096 slots -- some insertion must meet the probe cut.  Both rows
    are appended to the overflow list and decided from tables in the workspace; later iterations (the cliques have merged) fit the LDS table
    again, and the second case runs coarse levels after it."""
    from dynaalign_amd import device
    n, hubs = 4500, np.array([303, 1327])
    assert n > device.LOUVAIN_DIRECT_MAX and n - 1 > device.LOUVAIN_LDS_SLOTS > device.LOUVAIN_LDS_MAX
    assert all(vertex_class(int(h), seed) == 0 for h in hubs)
    csr = upload(*two_hub_graph(n, hubs))
    assert sorted(np.diff(host_csr(csr)[0]).tolist())[-2:] == [n - 1, n - 1]
    got = assert_equals_model(da, csr, np.arange(201, dtype=np.float64) / 200, res, seed)
    assert got[2] >= 2


def test_isolated_vertex_and_empty_graphs(da):
    csr, values = edge_list_csr(da, 6, [0, 0, 1, 4, 2], [1, 2, 2, 5, 2], [1.0, 1.0, 0.5, 0.25, 1.0])     # vertex 3: no edge, no loop
    got = assert_equals_model(da, csr, values)
    assert int((got[0] == got[0][3]).sum()) == 1 and got[0][4] == got[0][5]
    csr, values = edge_list_csr(da, 5, [], [], [])                                                      # nnz = 0, no loops: no weight at all
    got = assert_equals_model(da, csr, values)
    assert (got[0].tolist(), got[1], got[2], got[3]) == ([1, 2, 3, 4, 5], 0.0, 0, [])
    csr, values = edge_list_csr(da, 3, [0, 1, 2], [0, 1, 2], [1.0, 1.0, 1.0])                            # nnz = 0, loops only
    got = assert_equals_model(da, csr, values)
    assert (got[0].tolist(), got[2], got[3]) == ([1, 2, 3], 1, [1])
    csr, values = edge_list_csr(da, 2, [0], [1], [0.5])
    assert assert_equals_model(da, csr, values)[0].tolist() == [1, 1]
    csr, values = edge_list_csr(da, 1, [0], [0], [1.0])
    assert assert_equals_model(da, csr, values)[0].tolist() == [1]


# ------------------------------------------------------------------ determinism

def test_two_calls_agree_and_louvain_device_takes_any_edge_order(da):
    from dynaalign_amd import device
    n = 400
    ei, ej, ew = planted(n, 8, .3, .02, 1)
    csr, values = edge_list_csr(da, n, ei, ej, ew)
    a = device.louvain_csr(*csr, values, seed=7)
    b = device.louvain_csr(*csr, values, seed=7)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    rng = np.random.RandomState(3)
    perm = rng.permutation(len(ei))
    flip = rng.rand(len(ei)) < 0.5
    m, q = da.louvain_device(n, np.where(flip, ej, ei)[perm], np.where(flip, ei, ej)[perm], ew[perm], seed=7, return_modularity=True)
    assert np.array_equal(m, a[0]) and q == a[1]
    assert np.array_equal(da.louvain_device(n, ei, ej, ew, seed=7), a[0])


# ------------------------------------------------------------------ refusals (k_lv_validate, before any kernel indexes by these values)

@pytest.mark.parametrize("what", ["descending", "repeated", "diagonal", "code", "neighbour"])
def test_validate_refuses(da, what):
    import torch
    from dynaalign_amd import _capi
    lib = _capi.load()
    n, values = 4, np.array([0.5, 1.0])
    ptr = np.array([0, 2, 4, 6, 8], np.int64)
    adj = np.array([1, 2, 0, 3, 0, 3, 1, 2], np.int32)              # a canonical 4-cycle 0-1-3-2-0
    codes = np.zeros(8, np.uint16)
    if what == "descending":
        adj[0:2] = [2, 1]
    elif what == "repeated":
        adj[0:2] = [1, 1]
    elif what == "diagonal":
        adj[0:2] = [0, 1]
    elif what == "code":
        codes[5] = 2
    else:
        adj[7] = n
    t = upload(ptr, adj, codes, np.full(n, 0xFFFF, np.uint16))
    nbytes = lib.da_dev_louvain_workspace_bytes(n, 8)
    work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    member = torch.zeros(n, dtype=torch.int32, device="cuda")
    rc = lib.da_dev_louvain_csr(n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), values.ctypes.data, len(values), 1.05, 0,
                                work.data_ptr(), nbytes, member.data_ptr(), None, None, None, torch.cuda.current_stream().cuda_stream)
    assert rc == _capi.DA_ERR_BAD_ARG


# ------------------------------------------------------------------ the recursion

def test_clusterbreak_on_the_device_equals_the_model_as_cluster_fn(da, h3n2):
    import oracle_lib as O
    seqs, sess = h3n2
    seeds = O.seeds(12345, 200)

    def sim(x):
        rc, M = O.similarity_mh(x, 4, 200, seeds)
        assert rc == 0
        return M
    dev = da.clusterbreak(seqs, thresh_p=0.8, size_max=100, size_min=3, session=sess, louvain="device", louvain_device_min_nnz=0, cluster_seed=42)
    ref = da.clusterbreak(seqs, thresh_p=0.8, size_max=100, size_min=3, sim_fn=sim, cluster_fn=da.louvain_sync_dense, cluster_seed=42)
    assert dev["clustered_seq"].tolist() == ref["clustered_seq"].tolist()
    assert dev["filtered_seq"] == ref["filtered_seq"]
    assert (dev.calls, dev.convergence) == (ref.calls, ref.convergence) and dev.calls >= 5
    assert len(dev.levels) == len(ref.levels)
    for la, lb in zip(dev.levels, ref.levels):
        for key in ("itr", "n", "edges", "clusters", "oversize"):
            assert la[key] == lb[key], (key, la, lb)
        assert la["threshold"] == lb["threshold"] or (np.isnan(la["threshold"]) and np.isnan(lb["threshold"]))
    sizes = np.unique(dev["clustered_seq"][:, 1], return_counts=True)[1]
    assert sizes.min() >= 3 and sizes.max() <= 100
    # a threshold above every level: all levels take the host Louvain, and the result is the default's
    host = da.clusterbreak(seqs, thresh_p=0.8, size_max=100, size_min=3, session=sess, cluster_seed=42)
    same = da.clusterbreak(seqs, thresh_p=0.8, size_max=100, size_min=3, session=sess, louvain="host", cluster_seed=42)
    high = da.clusterbreak(seqs, thresh_p=0.8, size_max=100, size_min=3, session=sess, louvain="device", louvain_device_min_nnz=1 << 40, cluster_seed=42)
    for other in (same, high):
        assert other["clustered_seq"].tolist() == host["clustered_seq"].tolist() and other["filtered_seq"] == host["filtered_seq"]
        assert other.calls == host.calls


@pytest.mark.parametrize("kw", [{"knn": 5}, {"knn": 5, "knn_lsh": (20, 5)}])
def test_clusterbreak_on_the_device_with_knn_graphs(da, h3n2, kw):
    """the kNN forms of the recursion take their CSR from knn_csr_device / lsh_knn_csr_device: every sequence is clustered or filtered, the
    sizes are bounded, and two runs agree"""
    seqs, sess = h3n2
    a = da.clusterbreak(seqs, size_max=100, size_min=3, session=sess, louvain="device", louvain_device_min_nnz=0, cluster_seed=42, **kw)
    b = da.clusterbreak(seqs, size_max=100, size_min=3, session=sess, louvain="device", louvain_device_min_nnz=0, cluster_seed=42, **kw)
    assert a["clustered_seq"].tolist() == b["clustered_seq"].tolist() and a["filtered_seq"] == b["filtered_seq"] and a.calls == b.calls
    assert sorted(a["clustered_seq"][:, 0].tolist() + a["filtered_seq"]) == sorted(seqs)
    sizes = np.unique(a["clustered_seq"][:, 1], return_counts=True)[1]
    assert a.convergence == 1 and sizes.min() >= 3 and sizes.max() <= 100
