"""CPU tests of the connected components: the numpy definition (components_dense) against an independent breadth-first search, the host
union-find (da_components through components()) against the definition, the C ABI's symbols and argument checks -- every refusal arrives
before a device is needed -- the exports, and components as clusterbreak's cluster_fn.  On a machine with a device the ACCEPTED cases of
the validation test run the LSH pipeline on two short strings, as those of test_lsh_cpu.py do; here only the status is looked at."""
import ctypes
from collections import deque

import numpy as np
import pytest

import oracle_lib as O

CC_SYMBOLS = ["da_components", "da_dev_components_workspace_bytes", "da_dev_components_edges", "da_dev_components_csr", "da_dev_lsh_components",
              "da_similarity_mh_lsh_components"]
NEW_NAMES = ["components", "components_dense", "components_device", "similarityMH_lsh_components", "lsh_components_dense"]
OK, EMPTY, BAD_K, BAD_NHASH, NO_DEVICE, UNSUPPORTED, BAD_ARG = 0, 1, 2, 3, 8, 10, 11


def bfs(n, ei, ej):
    """The definition, the slow way: adjacency sets, a search from every vertex not reached yet in ascending order -- the start of a search
    is its component's smallest vertex, so the searches number the components by first appearance."""
    nb = [set() for _ in range(n)]
    for a, b in zip(ei, ej):
        a, b = int(a), int(b)
        assert 0 <= a < n and 0 <= b < n
        nb[a].add(b)
        nb[b].add(a)
    member = [0] * n
    count = 0
    for s in range(n):
        if member[s]:
            continue
        count += 1
        member[s] = count
        todo = deque([s])
        while todo:
            v = todo.popleft()
            for u in nb[v]:
                if not member[u]:
                    member[u] = count
                    todo.append(u)
    return member, count


def random_graph(seed, n, m):
    """m edges on n vertices: either orientation, with repeats and self-loops mixed in"""
    rng = np.random.default_rng(seed)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    ei = rng.integers(0, n, m).astype(np.int32)
    ej = rng.integers(0, n, m).astype(np.int32)
    if m >= 4:
        ei[1], ej[1] = ej[0], ei[0]               # the first edge again, turned round
        ei[2], ej[2] = ei[0], ej[0]               # and repeated
        ej[3] = ei[3]                             # a self-loop
    return ei, ej


GRAPHS = [(0, 0), (1, 0), (1, 3), (2, 0), (2, 1), (2, 5), (50, 0), (50, 20), (50, 60), (300, 100), (300, 250), (300, 900)]


def fixed_graphs():
    out = [("random n=%d m=%d" % (n, m), n) + random_graph(1000 + 7 * n + m, n, m) for n, m in GRAPHS]
    path = np.arange(9999, 0, -1, dtype=np.int32)                              # 0-1-...-9999, listed from the far end first
    out.append(("path", 10000, path, path - 1))
    star = np.arange(0, 2000, dtype=np.int32)                                  # the centre is the largest index
    out.append(("star", 2001, np.full(2000, 2000, np.int32), star))
    out.append(("loops only", 5, np.arange(5, dtype=np.int32), np.arange(5, dtype=np.int32)))
    return out


@pytest.fixture(scope="module")
def lib(built):
    from dynaalign_amd import _capi
    return _capi.load()


def check(got, want_member, want_count, n):
    member, count = got
    assert member.dtype == np.int32 and member.shape == (n,) and isinstance(count, int)
    assert member.tolist() == want_member and count == want_count
    assert np.bincount(member, minlength=1)[1:].sum() == n and (count == 0 or member.max() == count)


def test_dense_definition_against_a_breadth_first_search():
    import dynaalign_amd as da
    for name, n, ei, ej in fixed_graphs():
        want = bfs(n, ei, ej)
        check(da.components_dense(n, ei, ej), *want, n)
        if len(ei):                               # another order and the other orientation: the same labels
            p = np.random.default_rng(5).permutation(len(ei))
            check(da.components_dense(n, ej[p], ei[p]), *want, n)
            check(da.components_dense(n, ei[::-1], ej[::-1]), *want, n)
    # by hand: {0, 1}, {2}, {3}, {4, 5}: the minima are 0, 2, 3, 4
    assert da.components_dense(6, [5, 1, 3], [4, 0, 3])[0].tolist() == [1, 1, 2, 3, 4, 4]
    assert da.components_dense(4, [], [])[0].tolist() == [1, 2, 3, 4]
    for bad in (([0], [3]), ([-1], [0]), ([3], [0])):
        with pytest.raises(ValueError):
            da.components_dense(3, *bad)
    with pytest.raises(ValueError):
        da.components_dense(0, [0], [0])
    with pytest.raises(ValueError):
        da.components_dense(3, [0, 1], [1])


def test_host_union_find_equals_the_definition(lib):
    import dynaalign_amd as da
    for name, n, ei, ej in fixed_graphs():
        want_member, want_count = da.components_dense(n, ei, ej)
        check(da.components(n, ei, ej, return_count=True), want_member.tolist(), want_count, n)
        if len(ei):
            p = np.random.default_rng(6).permutation(len(ei))
            check(da.components(n, ej[p], ei[p], return_count=True), want_member.tolist(), want_count, n)
        # the cluster_fn calling convention: weights and seed are taken and ignored, the membership alone comes back
        got = da.components(n, ei, ej, np.ones(len(ei)), seed=9, weights=False)
        assert isinstance(got, np.ndarray) and got.tolist() == want_member.tolist()


def test_symbols_version_and_sizes(lib):
    from dynaalign_amd import _capi
    declared = _capi.header_symbols()
    for s in CC_SYMBOLS:
        assert s in declared and s in _capi.SIGNATURES and hasattr(lib, s), s
    assert lib.da_abi_version() == 2
    assert "#define DA_ABI_VERSION 2" in open(_capi.HEADER_PATH).read()
    sizes = [lib.da_dev_components_workspace_bytes(n) for n in (-5, 0, 1, 2, 1000, 1001, 10 ** 6, 10 ** 8, 2 ** 31 - 16, 2 ** 31, 2 ** 40)]
    assert sizes[0] > 0 and sizes == sorted(sizes)                              # monotone, and no device was needed
    assert sizes[4] >= 1000 * 12 and sizes[6] >= 10 ** 6 * 12                   # parent, flags and scan output: 4 bytes each
    assert sizes[-1] == sizes[-2] == sizes[-3]                                  # clamped to the largest n the calls take


def err(lib):
    return lib.da_last_error().decode("latin-1")


def test_host_call_refuses_bad_arguments(lib):
    e = np.zeros(4, np.int32)
    m = np.zeros(4, np.int32)
    c = np.full(1, -1, np.int64)
    E, M, C = e.ctypes.data, m.ctypes.data, c.ctypes.data
    assert lib.da_components(-1, 0, E, E, M, C) == BAD_ARG
    assert lib.da_components(3, -1, E, E, M, C) == BAD_ARG
    assert lib.da_components(2 ** 31, 0, E, E, M, C) == BAD_ARG
    assert lib.da_components(3, 0, None, None, M, None) == BAD_ARG and err(lib) == "NULL pointer"
    assert lib.da_components(3, 0, None, None, None, C) == BAD_ARG and err(lib) == "NULL membership buffer"
    assert lib.da_components(3, 2, None, E, M, C) == BAD_ARG and err(lib) == "NULL edge arrays"
    assert lib.da_components(3, 2, E, None, M, C) == BAD_ARG
    assert c[0] == -1                                                            # nothing was written by a refused call
    assert lib.da_components(0, 0, None, None, None, C) == OK and c[0] == 0      # n == 0
    assert lib.da_components(3, 0, None, None, M, C) == OK and c[0] == 3 and m[:3].tolist() == [1, 2, 3]
    for a, b in ((3, 0), (0, 3), (-1, 0), (0, -1)):
        i, j = np.array([0, a], np.int32), np.array([1, b], np.int32)
        assert lib.da_components(3, 2, i.ctypes.data, j.ctypes.data, M, C) == BAD_ARG
        assert err(lib) == "components: edge 1 (%d, %d) has an endpoint outside [0, 3)" % (a, b)
    import dynaalign_amd as da
    with pytest.raises(da.DynaAlignError) as ei:
        da.components(3, [0], [3])
    assert ei.value.code == BAD_ARG


def test_device_calls_refuse_bad_arguments_before_the_device(lib):
    """NULL pointers, negative sizes and a short workspace: the documented codes, with or without a device.  The pointers handed over
    are never dereferenced: every call here is refused, or returns at n == 0."""
    c = np.full(1, -1, np.int64)
    C = c.ctypes.data
    P = 256                                                                      # stands for a device pointer; never read
    need = lib.da_dev_components_workspace_bytes(10)
    edges = lib.da_dev_components_edges
    assert edges(P, P, None, 0, 5, -1, P, need, P, None, C, None) == BAD_ARG
    assert edges(P, P, None, 0, -1, 10, P, need, P, None, C, None) == BAD_ARG and err(lib) == "negative shape"
    assert edges(P, P, None, 0, 5, 10, P, need, P, None, None, None) == BAD_ARG and err(lib) == "NULL pointer"
    assert edges(P, P, None, 0, 5, 10, None, need, P, None, C, None) == BAD_ARG and err(lib) == "NULL device pointer"
    assert edges(P, P, None, 0, 5, 10, P, need, None, None, C, None) == BAD_ARG and err(lib) == "NULL device pointer"
    assert edges(None, P, None, 0, 5, 10, P, need, P, None, C, None) == BAD_ARG and err(lib) == "NULL device pointer"
    assert edges(P, None, None, 0, 5, 10, P, need, P, None, C, None) == BAD_ARG
    assert edges(P, P, None, 0, 5, 10, P, need - 1, P, None, C, None) == BAD_ARG and err(lib) == "components: workspace too small"
    assert edges(P, P, None, 0, 5, 2 ** 31, P, 1 << 40, P, None, C, None) == UNSUPPORTED
    c[0] = -1
    assert edges(None, None, None, 0, 0, 0, None, 0, None, None, C, None) == OK and c[0] == 0      # n == 0
    csr = lib.da_dev_components_csr
    assert csr(-1, P, P, 1, P, need, P, None, C, None) == BAD_ARG
    assert csr(10, P, P, 1, P, need, P, None, None, None) == BAD_ARG and err(lib) == "NULL pointer"
    assert csr(10, None, P, 1, P, need, P, None, C, None) == BAD_ARG and err(lib) == "NULL device pointer"
    assert csr(10, P, P, 1, None, need, P, None, C, None) == BAD_ARG
    assert csr(10, P, P, 1, P, need, None, None, C, None) == BAD_ARG
    assert csr(10, P, P, 1, P, need - 1, P, None, C, None) == BAD_ARG and err(lib) == "components: workspace too small"
    c[0] = -1
    assert csr(0, None, None, 1, None, 0, None, None, C, None) == OK and c[0] == 0
    lsh = lib.da_dev_lsh_components
    big = 1 << 30
    assert lsh(P, -1, 8, 8, 2, 4, 0.5, 100, P, big, P, None, C, None) == BAD_ARG
    assert lsh(P, 10, 8, 8, 2, 4, 0.5, 100, P, big, P, None, None, None) == BAD_ARG and err(lib) == "NULL pointer"
    assert lsh(P, 10, 8, 0, 2, 4, 0.5, 100, P, big, P, None, C, None) == BAD_NHASH
    assert lsh(None, 10, 8, 8, 2, 4, 0.5, 100, P, big, P, None, C, None) == BAD_ARG and err(lib) == "NULL device pointer"
    assert lsh(P, 10, 7, 8, 2, 4, 0.5, 100, P, big, P, None, C, None) == BAD_ARG and err(lib) == "ld_sig (7) < n_hash (8)"
    assert lsh(P, 10, 8, 8, 3, 4, 0.5, 100, P, big, P, None, C, None) == BAD_ARG and err(lib) == "bands * rows = 12 exceeds n_hash = 8"
    assert lsh(P, 10, 8, 8, 2, 4, 1.5, 100, P, big, P, None, C, None) == BAD_ARG and err(lib) == "the threshold must be in [0, 1]"
    assert lsh(P, 10, 8, 8, 2, 4, 0.5, -1, P, big, P, None, C, None) == BAD_ARG and err(lib) == "max_candidates must be >= 0 (got -1)"
    assert lsh(P, 10, 8, 8, 2, 4, 0.5, 100, None, big, P, None, C, None) == BAD_ARG and err(lib) == "NULL device pointer"
    assert lsh(P, 10, 8, 8, 2, 4, 0.5, 100, P, big, None, None, C, None) == BAD_ARG
    short = lib.da_dev_lsh_workspace_bytes(10, 2) + need - 1
    assert lsh(P, 10, 8, 8, 2, 4, 0.5, 100, P, short, P, None, C, None) == BAD_ARG and err(lib).startswith("lsh: workspace too small")
    c[0] = -1
    assert lsh(None, 0, 8, 8, 2, 4, 0.5, 100, None, 0, None, None, C, None) == OK and c[0] == 0


def raw_edges(lib, seqs, k, nh, bands, rows, thr, maxc=1 << 32, *, seeds=True, offsets=True, off=None, out=True, count=True):
    """da_similarity_mh_lsh_edges_begin through ctypes -> (status, text); a handle that came back is freed"""
    res, o = O.pack(seqs)
    if off is not None:
        o = np.asarray(off, np.int64)
    sv = np.zeros(max(nh, 1), np.uint32)
    h = ctypes.c_void_p()
    cnt = np.zeros(1, np.int64)
    rc = lib.da_similarity_mh_lsh_edges_begin(res.ctypes.data, o.ctypes.data if offsets else None, len(seqs), k, nh, sv.ctypes.data if seeds else None,
                                              bands, rows, thr, maxc, ctypes.addressof(h) if out else None, cnt.ctypes.data if count else None)
    if rc == OK:
        lib.da_edges_free(h)
    return rc, lib.da_last_error().decode("latin-1") if rc else ""


def raw_components(lib, seqs, k, nh, bands, rows, thr, maxc=1 << 32, *, seeds=True, offsets=True, off=None, out=True, count=True):
    """da_similarity_mh_lsh_components on the same arguments -> (status, text)"""
    res, o = O.pack(seqs)
    if off is not None:
        o = np.asarray(off, np.int64)
    sv = np.zeros(max(nh, 1), np.uint32)
    member = np.zeros(max(len(seqs), 1), np.int32)
    cnt = np.zeros(1, np.int64)
    rc = lib.da_similarity_mh_lsh_components(res.ctypes.data, o.ctypes.data if offsets else None, len(seqs), k, nh, sv.ctypes.data if seeds else None,
                                             bands, rows, thr, maxc, member.ctypes.data if out else None, cnt.ctypes.data if count else None)
    return rc, lib.da_last_error().decode("latin-1") if rc else ""


def test_host_boundary_checks_as_the_edge_form_does(lib, kats):
    """the same bad inputs into both calls: the same code and the same text, whichever check comes first"""
    e = kats["mh_errors"]
    two = ["ACDEFGHIK", "ACDEFGHIR"]
    nan = float("nan")
    cases = [(([], 0, 0, 0, 0, nan, -1), dict(seeds=False, offsets=False, out=False)),
             ((two, 0, 0, 0, 0, nan, -1), dict(seeds=False, offsets=False)),
             ((two, -2, 8, 2, 4, 0.5), {}),
             ((two, 4, 0, 0, 0, nan, -1), dict(seeds=False, offsets=False)),
             ((two, 4, -5, 2, 4, 0.5), {}),
             ((two, 4, 8, 0, 0, nan, -1), dict(off=[3, 2, 1], seeds=False)),
             ((two, 4, 8, 0, 0, nan, -1), dict(off=[3, 2, 1], out=False)),
             ((two, 4, 8, 0, 0, nan, -1), dict(off=[3, 2, 1], count=False)),
             ((two, 4, 8, 0, 0, nan, -1), dict(offsets=False)),
             ((two, 4, 8, 0, 0, nan, -1), dict(off=[0, 9, 5])),
             ((two, 4, 8, 0, 0, nan, -1), dict(off=[1, 9, 18]))]
    for nh in (8, 70000):
        cases += [((two, 4, nh, 0, 0, nan, -1), {}), ((two, 4, nh, -3, 4, 0.5), {}), ((two, 4, nh, 2, 0, nan, -1), {}),
                  ((two, 4, nh, nh // 4 + 1, 4, nan, -1), {}), ((two, 4, nh, 1, nh + 1, nan, -1), {}), ((two, 4, nh, 2, 4, 0.5, -1), {})]
        cases += [((two, 4, nh, 2, 4, thr, -1), {}) for thr in (nan, -0.001, 1.001, float("inf"))]
    cases.append(((two, 4, 65536, 2, 4, 0.5), {}))
    seen = set()
    for args, kw in cases:
        want = raw_edges(lib, *args, **kw)
        assert want[0] != OK
        assert raw_components(lib, *args, **kw) == want, (args, kw)
        seen.add(want)
    # the cases are not one refusal many times over: the texts of similarityMH, the pointer and offset checks, every LSH argument, the limit
    assert {(EMPTY, e["empty"]), (BAD_K, e["k"]), (BAD_NHASH, e["n_hash"]), (BAD_ARG, "NULL pointer"), (BAD_ARG, "offsets is NULL"),
            (BAD_ARG, "bands must be >= 1 (got 0)"), (BAD_ARG, "rows must be >= 1 (got 0)"), (BAD_ARG, "the threshold must be in [0, 1]"),
            (BAD_ARG, "max_candidates must be >= 0 (got -1)"),
            (UNSUPPORTED, "the LSH edge list counts in 16 bits: n_hash <= 65535 (got 65536)")} <= seen
    # accepted arguments: the pipeline on a machine with a device, DA_ERR_NO_DEVICE without one -- after every check
    want = OK if lib.da_device_count() > 0 else NO_DEVICE
    for args in ((two, 4, 8, 2, 4, 0.5), (two, 4, 8, 8, 1, 0.0), (two, 4, 8, 1, 8, 1.0), (["ACDEFGHIK"], 4, 8, 2, 4, 0.5, 0)):
        assert raw_components(lib, *args)[0] == want, args
    import dynaalign_amd as da
    for args, code, msg in [(([],), EMPTY, e["empty"]), ((two, 0), BAD_K, e["k"]), ((two, 4, 8, 3, 3), BAD_ARG, "bands * rows = 9 exceeds n_hash = 8")]:
        with pytest.raises(da.DynaAlignError) as ei:
            da.similarityMH_lsh_components(*args, seed=1)
        assert (ei.value.code, str(ei.value)) == (code, msg), args


def test_exports():
    import dynaalign_amd as da
    import importlib
    from dynaalign_amd import device, session
    cb = importlib.import_module("dynaalign_amd.clusterbreak")        # the package exports a function of the same name
    for name in NEW_NAMES:
        assert name in da.__all__ and callable(getattr(da, name)), name
    for name in ("components", "components_dense", "components_device"):
        assert name in cb.__all__
    for name in ("components_workspace_bytes", "components_edges", "components_csr", "lsh_components"):
        assert callable(getattr(device, name)), name
    for name in ("lsh_components", "components"):
        assert callable(getattr(session.MinHashSession, name)), name


def test_lsh_components_dense_is_the_components_of_the_dense_edges():
    import dynaalign_amd as da
    rng = np.random.default_rng(3)
    sig = rng.integers(0, 2 ** 32, (12, 8), dtype=np.uint64).astype(np.uint32)
    sig[1, 0:4] = sig[0, 0:4]                     # 0 - 1 through band 0 (4 of 8 columns: 0.5)
    sig[2, 4:8] = sig[1, 4:8]                     # 1 - 2 through band 1
    sig[5, 0:4] = sig[4, 0:4]                     # 4 - 5
    i, j, _ = da.lsh_edges_dense(sig, 2, 4, 0.5)
    member, count = da.lsh_components_dense(sig, 2, 4, 0.5)
    assert (member.tolist(), count) == bfs(12, i, j)
    assert member.tolist() == [1, 1, 1, 2, 3, 3, 4, 5, 6, 7, 8, 9] and count == 9
    assert da.lsh_components_dense(sig, 2, 4, 0.75)[1] == 12                    # nothing reaches 6 of 8 columns


def fixed_matrix():
    """9 peptides: p0..p3 pairwise 0.9, p4..p6 pairwise 0.8, everything else 0.2 or 0.1.  Of the 36 pairs 27 lie below 0.8, so the type-7
    quantile at 0.8 (position 29 of the sorted values) is 0.8: the graph keeps the two blocks and nothing else."""
    names = ["p%d" % t for t in range(9)]
    S = np.full((9, 9), 0.2)
    S[7, :] = S[:, 7] = S[8, :] = S[:, 8] = 0.1
    S[:4, :4] = 0.9
    S[4:7, 4:7] = 0.8
    np.fill_diagonal(S, 1.0)
    where = {p: t for t, p in enumerate(names)}

    def sim(pep):
        idx = [where[p] for p in pep]
        return S[np.ix_(idx, idx)]
    return names, sim


def test_components_as_the_cluster_fn_of_clusterbreak(lib):
    import dynaalign_amd as da
    names, sim = fixed_matrix()
    for fn in (da.components, lambda n, i, j, w, seed=0, weights=True: da.components_dense(n, i, j)[0]):
        r = da.clusterbreak(names, thresh_p=0.8, size_max=10, size_min=3, sim_fn=sim, cluster_fn=fn)
        assert isinstance(r, dict) and set(r) >= {"clustered_seq", "filtered_seq"}
        assert r["clustered_seq"].tolist() == [["p0", "1.1"], ["p1", "1.1"], ["p2", "1.1"], ["p3", "1.1"], ["p4", "1.2"], ["p5", "1.2"], ["p6", "1.2"]]
        assert r["filtered_seq"] == ["p7", "p8"]
        assert (r.calls, r.convergence) == (1, 1)
