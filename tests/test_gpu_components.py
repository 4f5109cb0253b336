"""GPU tests of the connected components: the device calls against the numpy definition (clusterbreak.components_dense), labels and sizes
element for element.  Every shape is small: what a kernel can get wrong shows at a path that is as deep as it is long, a star whose centre
is the largest index, rows of 1 / 64 / 65 / > 256 entries, more vertices than a launch has threads (DYNAALIGN_CC_BLOCKS caps the
workgroups, so that a graph of a few thousand vertices takes many grid-stride passes), and LSH candidate graphs whose components are
planted.  Argument errors are argument errors: no test builds anything that would index out of range if the validation were missing."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BAD_ARG = 11
SEED = 12345


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    from dynaalign_amd import _capi
    assert _capi.load().da_device_count() > 0
    return dynaalign_amd


def dev(a, dtype=torch.int32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def check_edges(da, n, ei, ej, **kw):
    """device.components_edges with sizes == components_dense, element for element"""
    from dynaalign_amd import device
    want, want_count = da.components_dense(n, ei, ej)
    member, count, sizes = device.components_edges(dev(ei), dev(ej), n, sizes=True, **kw)
    assert member.dtype == np.int32 and member.shape == (n,) and sizes.dtype == np.int32
    assert count == want_count and np.array_equal(member, want)
    assert np.array_equal(sizes, np.bincount(want, minlength=1)[1:])
    again, count2 = device.components_edges(dev(ei), dev(ej), n, **kw)            # without sizes: the same labels
    assert count2 == count and np.array_equal(again, member)
    return member, count


# ---- the edge-list form ---------------------------------------------------------------------------------------------------------------------
def path_graph(n, order):
    a = np.arange(n - 1, 0, -1, dtype=np.int32)                                   # far end first: every hook but the last meets a root
    b = a - 1
    if order == "shuffled":
        p = np.random.default_rng(11).permutation(n - 1)
        a, b = a[p], b[p]
        flip = np.random.default_rng(12).random(n - 1) < 0.5
        a, b = np.where(flip, b, a), np.where(flip, a, b)
    return a, b


def cliques_graph():
    """two cliques of 70 joined by one bridge, then 30 isolated vertices; the cliques' vertices are interleaved"""
    ids = np.random.default_rng(13).permutation(140)
    ca, cb = ids[:70], ids[70:]
    ei, ej = [], []
    for c in (ca, cb):
        a, b = np.triu_indices(70, 1)
        ei.append(c[a])
        ej.append(c[b])
    ei.append(ca[-1:])
    ej.append(cb[:1])
    return 170, np.concatenate(ei).astype(np.int32), np.concatenate(ej).astype(np.int32)


def forest_graph():
    rng = np.random.default_rng(14)
    return 70000, rng.integers(0, 70000, 35000).astype(np.int32), rng.integers(0, 70000, 35000).astype(np.int32)


def edge_cases():
    return {
        "one vertex": (1, np.zeros(0, np.int32), np.zeros(0, np.int32)),
        "loops only": (5, np.arange(5, dtype=np.int32), np.arange(5, dtype=np.int32)),
        "path far end first": (4097,) + path_graph(4097, "far"),
        "path shuffled": (4097,) + path_graph(4097, "shuffled"),
        "star": (4097, np.full(4096, 4096, np.int32), np.arange(4096, dtype=np.int32)),
        "cliques": cliques_graph(),
        "forest": forest_graph(),
    }


@pytest.mark.parametrize("name", list(edge_cases()))
def test_edge_list_equals_the_definition(da, name):
    n, ei, ej = edge_cases()[name]
    member, count = check_edges(da, n, ei, ej)
    if name == "one vertex":
        assert (member.tolist(), count) == ([1], 1)
    if name == "loops only":
        assert (member.tolist(), count) == ([1, 2, 3, 4, 5], 5)
    if name.startswith("path") or name == "star":
        assert count == 1
    if name == "cliques":
        assert count == 31
    if name == "forest":
        assert 35000 < count < 70000


def test_labels_do_not_depend_on_the_order_of_the_edges(da):
    n, ei, ej = forest_graph()
    first, count = check_edges(da, n, ei, ej)
    for seed in (1, 2):
        p = np.random.default_rng(seed).permutation(len(ei))
        again, count2 = check_edges(da, n, ej[p], ei[p])
        assert count2 == count and np.array_equal(again, first)


@pytest.mark.parametrize("blocks", ["1", "3"])
def test_many_grid_stride_passes(da, monkeypatch, blocks):
    """a launch of 1 or 3 workgroups: 256 or 768 threads for 4 097 vertices and 35 000 edges"""
    monkeypatch.setenv("DYNAALIGN_CC_BLOCKS", blocks)
    for name in ("path shuffled", "star", "cliques"):
        check_edges(da, *edge_cases()[name])
    n, ei, ej = forest_graph()
    check_edges(da, 9000, ei % 9000, ej % 9000)


def test_code_filter_cuts_one_list_at_three_thresholds(da):
    from dynaalign_amd import device
    rng = np.random.default_rng(15)
    n, m = 400, 330
    ei, ej = rng.integers(0, n, m).astype(np.int32), rng.integers(0, n, m).astype(np.int32)
    codes = rng.choice(np.array([10, 20, 30, 40000], np.uint16), m)               # 40000: above 2^15, codes are unsigned
    tc = torch.from_numpy(codes.view(np.int16)).cuda()
    parts = []
    for min_code in (10, 21, 31):                                                 # all edges; codes 30 and 40000; 40000 only
        keep = codes >= min_code
        want, want_count = da.components_dense(n, ei[keep], ej[keep])
        member, count, sizes = device.components_edges(dev(ei), dev(ej), n, codes=tc, min_code=min_code, sizes=True)
        assert count == want_count and np.array_equal(member, want) and np.array_equal(sizes, np.bincount(want)[1:])
        parts.append((member, count))
    assert parts[0][1] < parts[1][1] < parts[2][1] < n                            # strictly coarser to finer
    for (coarse, _), (fine, cf) in zip(parts, parts[1:]):                         # every finer component lies in one coarser component
        assert len(set(zip(fine.tolist(), coarse.tolist()))) == cf
    none, count = device.components_edges(dev(ei), dev(ej), n, codes=tc, min_code=40001)
    assert count == n and np.array_equal(none, np.arange(1, n + 1))
    same, count = device.components_edges(dev(ei), dev(ej), n, codes=tc, min_code=0)
    assert np.array_equal(same, parts[0][0])


# ---- the CSR form ---------------------------------------------------------------------------------------------------------------------------
def csr_edges():
    """(i <= j) list on 700 vertices: a hub of 300 leaves (a row of > 256 entries), one of 64 and one of 65, leaves (rows of 1 entry), a
    chain that ties the 65-hub to a far vertex, isolated vertices, and a few diagonal entries"""
    e = [(0, v) for v in range(1, 301)] + [(301, v) for v in range(302, 366)] + [(400, v) for v in range(401, 466)]
    e += [(v, v + 1) for v in range(470, 480)] + [(465, 470)] + [(500, 699), (501, 699), (600, 601)] + [(5, 5), (650, 650)]
    e = np.array(sorted(e), np.int32)
    return 700, e[:, 0].copy(), e[:, 1].copy()


def test_csr_rows_of_1_64_65_and_more_than_256_entries(da):
    from dynaalign_amd import device
    n, ei, ej = csr_edges()
    ev = torch.ones(len(ei), dtype=torch.int16, device="cuda")
    ptr, adj, _, _ = device.edges_to_csr(dev(ei), dev(ej), ev, len(ei), n)
    deg = np.diff(ptr.cpu().numpy())
    assert {0, 1, 64, 65} <= set(deg.tolist()) and deg.max() == 300 and deg[0] == 300 and deg[301] == 64 and deg[400] == 65
    want, want_count = da.components_dense(n, ei, ej)
    for symmetric in (True, False):
        member, count, sizes = device.components_csr(ptr, adj, symmetric=symmetric, sizes=True)
        assert count == want_count and np.array_equal(member, want), symmetric
        assert np.array_equal(sizes, np.bincount(want)[1:])
    # an asymmetric CSR -- every edge in the row of its smaller end only, the rows listed backwards -- taken as what it is
    up = ei != ej
    a, b = ei[up], ej[up]
    o = np.lexsort((-b, a))
    uptr = np.zeros(n + 1, np.int64)
    np.add.at(uptr, a + 1, 1)
    member, count = device.components_csr(dev(np.cumsum(uptr), torch.int64), dev(b[o]), symmetric=False)
    assert count == want_count and np.array_equal(member, want)
    # a CSR without any entry
    member, count = device.components_csr(torch.zeros(8, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"))
    assert count == 7 and member.tolist() == [1, 2, 3, 4, 5, 6, 7]


def test_csr_with_few_workgroups(da, monkeypatch):
    from dynaalign_amd import device
    monkeypatch.setenv("DYNAALIGN_CC_BLOCKS", "1")                                # one workgroup walks the three tiles of 256 rows
    n, ei, ej = csr_edges()
    ptr, adj, _, _ = device.edges_to_csr(dev(ei), dev(ej), torch.ones(len(ei), dtype=torch.int16, device="cuda"), len(ei), n)
    want, want_count = da.components_dense(n, ei, ej)
    for symmetric in (True, False):
        member, count = device.components_csr(ptr, adj, symmetric=symmetric)
        assert count == want_count and np.array_equal(member, want)


# ---- validation -----------------------------------------------------------------------------------------------------------------------------
def test_bad_endpoints_and_bad_row_pointers_are_argument_errors(da):
    from dynaalign_amd import device
    n = 300
    ei, ej = np.arange(0, 299, dtype=np.int32), np.arange(1, 300, dtype=np.int32)
    for pos, a, b in ((298, 0, n), (0, n, 1), (150, n, n)):                         # (300 words of parents: word n lies in the array's padding)
        xi, xj = ei.copy(), ej.copy()
        xi[pos], xj[pos] = a, b
        with pytest.raises(da.DynaAlignError) as e:
            device.components_edges(dev(xi), dev(xj), n)
        assert e.value.code == BAD_ARG and "outside [0, n)" in str(e.value)
    # an endpoint of a filtered edge is checked too
    codes = torch.zeros(299, dtype=torch.int16, device="cuda")
    xj = ej.copy()
    xj[10] = n
    with pytest.raises(da.DynaAlignError) as e:
        device.components_edges(dev(ei), dev(xj), n, codes=codes, min_code=5)
    assert e.value.code == BAD_ARG
    # row pointers: ptr[n] is the number of entries, every neighbour is in range and every pointer inside [0, nnz], but they decrease or
    # start behind 0
    adj = dev(np.array([1, 0, 3, 2], np.int32))
    for ptr in ([0, 3, 2, 4, 4], [1, 1, 2, 4, 4], [0, 4, 4, 3, 4]):
        with pytest.raises(da.DynaAlignError) as e:
            device.components_csr(dev(np.array(ptr, np.int64), torch.int64), adj, symmetric=False)
        assert e.value.code == BAD_ARG, ptr
    with pytest.raises(da.DynaAlignError) as e:                                   # a neighbour equal to n
        device.components_csr(dev(np.array([0, 1, 2, 3, 4], np.int64), torch.int64), dev(np.array([1, 0, 4, 2], np.int32)))
    assert e.value.code == BAD_ARG
    # the valid twin of the CSR above runs
    member, count = device.components_csr(dev(np.array([0, 1, 2, 3, 4], np.int64), torch.int64), adj)
    assert (member.tolist(), count) == ([1, 1, 2, 2], 2)


# ---- the LSH form on hand-built signatures --------------------------------------------------------------------------------------------------
N_HASH, BANDS, ROWS, THRESHOLD = 24, 6, 4, 0.25                                   # an edge needs 6 equal columns: one band and two more


def distinct_sig(seed, n):
    """pairwise-distinct uint32 values: no two rows agree anywhere until something is copied"""
    rng = np.random.default_rng(seed)
    return (rng.permutation(n * N_HASH).astype(np.uint32) * np.uint32(2654435761)).reshape(n, N_HASH)


def link(sig, a, b, band, strong=True):
    """row b takes band `band` of row a -- a candidate -- and, if strong, two columns of the band three further: 6 equal columns = 0.25.
    Without them the pair has 4 of 24 and stays below the threshold."""
    sig[b, band * ROWS:(band + 1) * ROWS] = sig[a, band * ROWS:(band + 1) * ROWS]
    if strong:
        t = (band + 3) % BANDS
        sig[b, t * ROWS:t * ROWS + 2] = sig[a, t * ROWS:t * ROWS + 2]


def small_planted():
    sig = distinct_sig(21, 14)
    for k in range(4):                            # a chain 0 - 1 - 2 - 3 - 4, every link through another band
        link(sig, k, k + 1, k)
    link(sig, 5, 6, 2, strong=False)              # shares a band, 4 / 24 < 0.25: must not link
    link(sig, 7, 8, 5)                            # a triple in one bucket of band 5
    link(sig, 7, 9, 5)
    return sig                                    # 10 .. 13: singletons


def large_planted():
    """3 000 rows: 1 000 groups of 2 or 3 rows -- chains through changing bands, every seventh group joined below the threshold only --
    then noise rows; the rows are shuffled so that a group's members lie far apart"""
    n = 3000
    sig = distinct_sig(22, n)
    row = 0
    for g in range(1000):
        size = 2 + g % 2
        for k in range(size - 1):
            link(sig, row + k, row + k + 1, (g + k) % BANDS, strong=g % 7 != 0)
        row += size
    assert row == 2500
    return sig[np.random.default_rng(23).permutation(n)]


def sig_tensor(sig):
    return torch.from_numpy(sig.view(np.int32)).cuda()


def check_lsh(da, sig):
    from dynaalign_amd import device
    n = len(sig)
    want, want_count = da.lsh_components_dense(sig, BANDS, ROWS, THRESHOLD)
    t = sig_tensor(sig)
    member, count, sizes = device.lsh_components(t, N_HASH, BANDS, ROWS, THRESHOLD, sizes=True)
    route = device.mh_lsh_last_route()
    assert member.dtype == np.int32 and count == want_count and np.array_equal(member, want)
    assert np.array_equal(sizes, np.bincount(want)[1:])
    ei, ej, _ = device.lsh_edges(t, N_HASH, BANDS, ROWS, THRESHOLD)
    edge_route = device.mh_lsh_last_route()
    from_edges, count_edges = da.components_dense(n, ei.cpu().numpy(), ej.cpu().numpy())
    assert count_edges == count and np.array_equal(from_edges, member)
    assert route == edge_route and route["edges"] == ei.numel() > n
    return want, want_count


def test_lsh_components_on_hand_built_signatures(da):
    sig = small_planted()
    want, want_count = da.lsh_components_dense(sig, BANDS, ROWS, THRESHOLD)
    # before the device is used: the comparison is not vacuous
    assert want_count >= 6 and want_count == 8
    assert want[5] != want[6]                                                     # the sub-threshold pair is split ...
    bi, bj, _ = da.lsh_edges_dense(sig, BANDS, ROWS, 0.0)
    assert (5, 6) in set(zip(bi.tolist(), bj.tolist()))                           # ... though it is a candidate
    assert len(set(want[:5].tolist())) == 1 and want[7] == want[8] == want[9] and len(set(want[10:].tolist())) == 4
    check_lsh(da, sig)


def test_lsh_components_on_three_thousand_planted_rows(da, monkeypatch):
    sig = large_planted()
    want, want_count = da.lsh_components_dense(sig, BANDS, ROWS, THRESHOLD)
    sizes = np.bincount(want)[1:]
    assert want_count > 1000 and {1, 2, 3} == set(sizes.tolist())
    check_lsh(da, sig)
    monkeypatch.setenv("DYNAALIGN_CC_BLOCKS", "2")                                # and with 8 waves for all the candidate slots
    check_lsh(da, sig)


def test_lsh_components_workspace_and_threshold_one(da):
    from dynaalign_amd import device
    sig = small_planted()
    sig[11] = sig[10]                                                             # an exact duplicate: the only edge left at 1.0
    t = sig_tensor(sig)
    need = device.lsh_workspace_bytes(len(sig), BANDS) + device.components_workspace_bytes(len(sig))
    with pytest.raises(da.DynaAlignError) as e:
        device.lsh_components(t, N_HASH, BANDS, ROWS, 1.0, work=torch.empty(need - 1, dtype=torch.uint8, device="cuda"))
    assert e.value.code == BAD_ARG
    work = torch.empty(need + 1, dtype=torch.uint8, device="cuda")[1:]            # any alignment
    member, count = device.lsh_components(t, N_HASH, BANDS, ROWS, 1.0, work=work)
    want, want_count = da.lsh_components_dense(sig, BANDS, ROWS, 1.0)
    assert count == want_count == 13 and np.array_equal(member, want) and member[10] == member[11]


# ---- session and host boundary --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def h3n2():
    from dynaalign_amd import synth
    res, off = synth.h3n2_like(300, 20)
    return list(dict.fromkeys(synth.to_strings(res, off)))


def test_host_boundary_equals_the_components_of_the_edge_call(da, h3n2):
    n = len(h3n2)
    assert n > 100
    for bands, rows, thr in ((12, 4, 0.5), (6, 8, 0.8)):
        _, ei, ej, _ = da.similarityMH_lsh_edges(h3n2, 4, 48, bands, rows, thr, seed=SEED)
        want, want_count = da.components_dense(n, ei, ej)
        member, count = da.similarityMH_lsh_components(h3n2, 4, 48, bands, rows, thr, seed=SEED)
        assert member.dtype == np.int32 and count == want_count and np.array_equal(member, want)
        assert 1 < count < n
        host, host_count = da.components(n, ei, ej, return_count=True)
        assert host_count == count and np.array_equal(host, member)


def test_session_components(da, h3n2):
    from dynaalign_amd import session
    s = session.MinHashSession(h3n2, 4, 48, seed=SEED, reserve=False)
    idx = np.random.RandomState(9).permutation(len(h3n2))[:151]
    for ix in (None, idx):
        m = len(h3n2) if ix is None else len(ix)
        _, ei, ej, _ = s.lsh_edges(12, 4, 0.5, idx=ix)
        want, want_count = da.components_dense(m, ei, ej)
        member, count = s.lsh_components(12, 4, 0.5, idx=ix)
        assert count == want_count and np.array_equal(member, want)
        _, ei, ej, _ = s.edges(ix, thresh_p=0.8)
        want, want_count = da.components_dense(m, ei, ej)
        member, count = s.components(ix, thresh_p=0.8)
        assert count == want_count and np.array_equal(member, want)
    sub = [h3n2[t] for t in idx]
    member, count = da.similarityMH_lsh_components(sub, 4, 48, 12, 4, 0.5, seed=s.seed)
    assert (count, member.tolist()) == (s.lsh_components(12, 4, 0.5, idx=idx)[1], s.lsh_components(12, 4, 0.5, idx=idx)[0].tolist())


def test_components_device_as_a_cluster_fn(da):
    n, ei, ej = cliques_graph()
    want, want_count = da.components_dense(n, ei, ej)
    got = da.components_device(n, ei, ej, np.ones(len(ei)), seed=3, weights=False)
    assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    member, count = da.components_device(n, ei, ej, return_count=True)
    assert count == want_count and np.array_equal(member, want)
    with pytest.raises(ValueError):
        da.components_device(n, [0], [n])
