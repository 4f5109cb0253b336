"""clusterbreak -- the caller of the hot path, restated (BASELINE config 5).

    clusterbreak(pep, thresh_p=0.8, size_max=10, size_min=3, max_itr=10000, sim_fn=..., cluster_fn=..., cluster_wt=True)
                                                                              reference R/clusterbreak.R:180-275
    netcluster(pepmat, ...)                                                   reference R/clusterbreak.R:112-136
    clusterconsensus(df)                                                      reference R/clusterbreak.R:309-320 (center-star, not DECIPHER)

Same argument names, defaults, messages and bookkeeping as the R functions.  Per recursion level
(``cluster_recursive``, R/clusterbreak.R:203-259):

    pep.sim   <- sim_fn(pep)                                          :217   the hot-path call
    threshold <- quantile(pep.sim[upper.tri(pep.sim)], thresh_p)      :219   R type 7
    pep.sim[pep.sim < threshold] <- 0                                 :221
    c.index   <- netcluster(pep.sim, ...)                             :222   upper triangle incl. the 1.0 diagonal
    sizes, id.itr (> size_max), id.rm (< size_min), labels "<itr>.<cluster>", recursion   :224-254

Three ways to produce a level's thresholded graph, with identical results:

  * ``sim_fn`` (the reference's contract): any function sequences -> dense symmetric matrix.  The three R
    statements above are restated literally in `threshold_edges_dense`.  Works with ``similarityMH`` /
    ``similarityNW`` of this package, or -- in the tests -- with the CPU oracle.
  * ``edges_fn``: any function sequences -> (threshold, i, j, weight), the same graph as an edge list (``similarityNW_edges_long``: the
    alignment identity of sequences up to 1024 residues, thresholded on the device).
  * ``session`` (device fast path): a `MinHashSession` keeps the signatures of all sequences in HBM; a level is
    K1b + K2 + histogram + exact type-7 quantile + edge extraction on the index subset (`MinHashSession.edges`),
    and only the surviving edges leave the GPU.  The dense matrix never exists (80 GB at N = 100k).

The default ``cluster_fn`` is `louvain` (resolution 1.05, the reference's default, :115-116/:186-187) on the
library's host-side multilevel implementation (`da_louvain`); igraph is not importable here and its result
depends on R's RNG stream, so memberships are reproducible given ``cluster_seed`` but are not igraph's.
"""
import sys
import time

import numpy as np

from . import _capi

__all__ = ["clusterbreak", "clusterconsensus", "netcluster", "louvain", "louvain_sync_dense", "louvain_device", "threshold_edges_dense",
           "components", "components_dense", "components_device", "ClusterbreakResult"]


def louvain(n, ei, ej, ew, resolution=1.05, seed=0, weights=True, return_modularity=False):
    """igraph::cluster_louvain(g, weights = E(g)$weight, resolution)$membership on an edge list (0-based,
    i == j = self-loop).  weights=False clusters the unweighted graph (a graph built with igraph_weight = FALSE; NOT what
    netcluster's cluster_weight = FALSE does with the default cluster_func -- see _run_cluster_fn).  Returns int32 ids
    starting at 1 (R's numbering)."""
    lib = _capi.load()
    ei = np.ascontiguousarray(ei, np.int32)
    ej = np.ascontiguousarray(ej, np.int32)
    ew = np.ascontiguousarray(ew, np.float64) if weights else np.ones(len(ei), np.float64)
    if not (len(ei) == len(ej) == len(ew)):
        raise ValueError("edge arrays differ in length")
    member = np.zeros(max(int(n), 1), np.int32)
    q = np.zeros(1, np.float64)
    lv = np.zeros(1, np.int32)
    _capi.check(lib.da_louvain(int(n), len(ei), ei.ctypes.data, ej.ctypes.data, ew.ctypes.data, float(resolution),
                               int(seed) & 0xFFFFFFFF, member.ctypes.data, q.ctypes.data if return_modularity else None,   # (the modularity is
                               lv.ctypes.data))                                                                           # a sweep over all edges)
    member = member[:int(n)]
    return (member, float(q[0])) if return_modularity else member


_louvain_host = louvain


def louvain_csr(n, ptr, adj, codes, loop_codes, values, resolution=1.05, seed=0, weights=True, return_modularity=False):
    """`louvain` on a graph that is already canonical (da_louvain_csr): symmetric CSR, weights as uint16 codes into `values`,
    self-loops per vertex as codes (0xFFFF = none).  What MinHashSession.edges_csr hands over -- sorted on the device, no host-side
    sort of the edge list.  weights=False clusters the unweighted graph (every code stands for 1.0).  Same result as `louvain`
    on the corresponding edge list."""
    lib = _capi.load()
    ptr = np.ascontiguousarray(ptr, np.int64)
    adj = np.ascontiguousarray(adj, np.int32)
    codes = np.ascontiguousarray(codes, np.uint16)
    loop_codes = np.ascontiguousarray(loop_codes, np.uint16)
    values = np.ascontiguousarray(values, np.float64) if weights else np.ones(len(values), np.float64)
    member = np.zeros(max(int(n), 1), np.int32)
    q = np.zeros(1, np.float64)
    lv = np.zeros(1, np.int32)
    _capi.check(lib.da_louvain_csr(int(n), ptr.ctypes.data, adj.ctypes.data, codes.ctypes.data, loop_codes.ctypes.data, values.ctypes.data,
                                   len(values), float(resolution), int(seed) & 0xFFFFFFFF, member.ctypes.data,
                                   q.ctypes.data if return_modularity else None, lv.ctypes.data))
    member = member[:int(n)]
    return (member, float(q[0])) if return_modularity else member


# ---- the synchronous Louvain: its definition (numpy) and the device call that reproduces it bit for bit ------------------------------------
LV_SCALE_BITS = 30        # every weight becomes the integer rint(w * 2**30); all sums of weights are exact 64-bit integers
LV_CLASSES = 8            # sub-rounds per iteration
LV_MAX_ITERATIONS = 64
LV_MAX_LEVELS = 32
LV_M2_LIMIT = 1 << 62
LOUVAIN_DEVICE_MIN_NNZ = 1 << 17   # clusterbreak(louvain="device"): smaller levels stay on the host


def _lv_quantise(ew):
    ew = np.ascontiguousarray(ew, np.float64)
    if not np.isfinite(ew).all():
        raise ValueError("edge weights must be finite")
    if (ew < 0).any():
        raise ValueError("edge weights must not be negative")
    return np.rint(ew * float(1 << LV_SCALE_BITS)).astype(np.int64)


def _lv_csr(n, ei, ej, wq):
    """symmetric adjacency without a diagonal (repeated edges summed) + the self-loop weight per vertex"""
    loop = np.zeros(n, np.int64)
    d = ei == ej
    np.add.at(loop, ei[d], wq[d])
    a = np.concatenate([ei[~d], ej[~d]]).astype(np.int64)
    b = np.concatenate([ej[~d], ei[~d]]).astype(np.int64)
    w = np.concatenate([wq[~d], wq[~d]])
    key = a * n + b
    o = np.argsort(key, kind="stable")
    key, w = key[o], w[o]
    uk, st = np.unique(key, return_index=True)
    w = np.add.reduceat(w, st) if len(w) else w
    ptr = np.zeros(n + 1, np.int64)
    np.add.at(ptr, uk // n + 1, 1)
    return np.cumsum(ptr), uk % n, w, loop


def _lv_modularity(m2, inn, tot, res):
    """Q = IN / m2 - res * (S / (m2 * m2)): IN and S = sum tot^2 exact integers (S has up to 124 bits), each converted to double once"""
    s = sum(int(t) * int(t) for t in tot.tolist())
    return float(inn) / float(m2) - res * (float(s) / (float(m2) * float(m2)))


def _lv_pass(ptr, adj, w, loop, res, seed, level):
    """one level on (ptr, adj, w, loop) -> (comm, moved_any, iterations, Q after the last iteration); m2 > 0"""
    n = len(ptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
    k = 2 * loop
    np.add.at(k, rows, w)
    m2 = int(k.sum())
    kf, m2f = k.astype(np.float64), float(m2)
    comm, tot, size = np.arange(n, dtype=np.int64), k.copy(), np.ones(n, np.int64)
    with np.errstate(over="ignore"):
        h = ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(int(seed) * 40503 + level)) >> np.uint64(7)) & np.uint64(7)
    h = h.astype(np.int64)
    loops2 = 2 * int(loop.sum())

    def quality():
        return _lv_modularity(m2, int(w[comm[rows] == comm[adj]].sum()) + loops2, tot, res)
    q_prev = q = quality()
    moved_any, iterations = False, 0
    for _ in range(LV_MAX_ITERATIONS):
        iterations += 1
        moved = 0
        for g in range(LV_CLASSES):
            vs = np.nonzero(h == g)[0]
            if len(vs) == 0:
                continue
            sel = h[rows] == g
            # (vertex, neighbour community, summed weight), the vertex's own community always among them (weight 0 when no neighbour is in it)
            r = np.concatenate([rows[sel], vs])
            c = np.concatenate([comm[adj[sel]], comm[vs]])
            ww = np.concatenate([w[sel], np.zeros(len(vs), np.int64)])
            key = r * n + c
            o = np.argsort(key, kind="stable")
            key, ww = key[o], ww[o]
            uk, st = np.unique(key, return_index=True)
            ws = np.add.reduceat(ww, st)
            rv, cc = uk // n, uk % n
            own = cc == comm[rv]
            t = tot[cc] - np.where(own, k[rv], 0)
            gain = ws.astype(np.float64) - ((res * t.astype(np.float64)) * kf[rv]) / m2f
            stay = np.empty(n, np.float64)
            stay[rv[own]] = gain[own]
            ok = ~own & (gain > stay[rv])
            ok &= ~((size[comm[rv]] == 1) & (size[cc] == 1) & (cc > comm[rv]))           # two lone vertices must not swap for ever
            rv, cc, gain = rv[ok], cc[ok], gain[ok]
            o = np.lexsort((cc, -gain, rv))                                                # largest gain, then the smaller community id
            rv, cc = rv[o], cc[o]
            first = np.ones(len(rv), bool)
            first[1:] = rv[1:] != rv[:-1]
            mv, mc = rv[first], cc[first]
            old = comm[mv]
            np.add.at(tot, old, -k[mv])
            np.add.at(tot, mc, k[mv])
            np.add.at(size, old, -1)
            np.add.at(size, mc, 1)
            comm[mv] = mc
            moved += len(mv)
        q = quality()
        if moved == 0:
            break
        moved_any = True
        if not q > q_prev:                 # the moves are kept (the host Louvain does the same)
            break
        q_prev = q
    return comm, moved_any, iterations, q


def _lv_aggregate(ptr, adj, w, loop, comm):
    n = len(ptr) - 1
    u, newc = np.unique(comm, return_inverse=True)
    nc = len(u)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
    a, b = newc[rows], newc[adj]
    nloop = np.zeros(nc, np.int64)
    np.add.at(nloop, newc, loop)
    d = a == b
    inner = np.zeros(nc, np.int64)
    np.add.at(inner, a[d], w[d])
    nloop += inner // 2                    # every internal edge was counted from both ends
    a, b, ww = a[~d], b[~d], w[~d]
    key = a * nc + b
    o = np.argsort(key, kind="stable")
    key, ww = key[o], ww[o]
    uk, st = np.unique(key, return_index=True)
    ws = np.add.reduceat(ww, st) if len(ww) else ww
    nptr = np.zeros(nc + 1, np.int64)
    np.add.at(nptr, uk // nc + 1, 1)
    return newc, np.cumsum(nptr), uk % nc, ws, nloop


def _lv_first_appearance(member):
    _, first, inv = np.unique(member, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(1, len(first) + 1)
    return rank[inv].astype(np.int32)


def louvain_sync_dense(n, ei, ej, ew, resolution=1.05, seed=0, weights=True, return_info=False):
    """The synchronous Louvain `louvain_device` runs on the GPU, as its definition in numpy (the ``cluster_fn`` calling convention; the
    device call reproduces membership, modularity, levels and iterations bit for bit).  NOT the host `louvain`: another clustering
    function with other memberships.

    Weights become integers rint(w * 2**30) and every sum of weights is an exact 64-bit integer.  Symmetric adjacency without a diagonal,
    self-loops per vertex, k_v = 2 loop_v + sum_u w(v, u), m2 = sum_v k_v.  A level starts from singletons; the vertices fall into 8
    classes h(v) = ((v * 2654435761 + seed * 40503 + level) >> 7) & 7 (uint64), and an iteration is 8 sub-rounds: the vertices of one
    class decide from the same snapshot, then all their moves are applied.  With C = comm[v] and g(w, t) = w - ((resolution * t) * k_v) / m2
    in doubles, v moves to the neighbouring community c != C of largest g(w(v, c), tot[c]) (ties: the smaller c) among those with
    g > g(w(v, C), tot[C] - k_v), a candidate being barred when size[C] == size[c] == 1 and c > C.  After an iteration
    Q = IN / m2 - resolution * (S / (m2 * m2)) from the exact internal weight IN and S = sum tot^2; the level stops when nothing moved,
    when Q did not strictly improve (the moves are kept), or after 64 iterations.  Communities are renumbered by ascending id, the graph is
    aggregated with integer sums, and levels repeat until one moves nothing, merges nothing, or 32 have run.

    Returns ids from 1 in order of first appearance; with return_info ``(membership, Q, levels, iterations)``: the number of levels run
    and the iterations of each."""
    n = int(n)
    ei = np.ascontiguousarray(ei, np.int64)
    ej = np.ascontiguousarray(ej, np.int64)
    ew = np.ascontiguousarray(ew, np.float64) if weights else np.ones(len(ei), np.float64)
    if not (len(ei) == len(ej) == len(ew)):
        raise ValueError("edge arrays differ in length")
    if n < 0:
        raise ValueError("n must not be negative")
    if len(ei) and (min(ei.min(), ej.min()) < 0 or max(ei.max(), ej.max()) >= n):
        raise ValueError("edge endpoint out of range")
    wq = _lv_quantise(ew)
    res = float(resolution)
    ptr, adj, w, loop = _lv_csr(n, ei, ej, wq)
    if len(adj) * int(wq.max(initial=0)) + 2 * int(loop.sum()) >= LV_M2_LIMIT:
        raise ValueError("total edge weight too large for exact 64-bit sums")
    member = np.arange(n, dtype=np.int64)
    k0 = 2 * loop
    np.add.at(k0, np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr)), w)
    q, iterations = 0.0, []
    if int(k0.sum()) > 0:
        for level in range(LV_MAX_LEVELS):
            comm, moved, its, q = _lv_pass(ptr, adj, w, loop, res, seed, level)
            iterations.append(its)
            if not moved:
                break
            newc, nptr, nadj, nw, nloop = _lv_aggregate(ptr, adj, w, loop, comm)
            member = newc[member]
            merged = len(nptr) < len(ptr)
            ptr, adj, w, loop = nptr, nadj, nw, nloop
            if not merged:
                break
    out = _lv_first_appearance(member)
    return (out, q, len(iterations), iterations) if return_info else out


def canonical_csr(n, ei, ej, ew):
    """an edge list (i == j = self-loop, either orientation, any order) as the canonical symmetric CSR `louvain_csr` and
    `device.louvain_csr` take: (ptr, adj, codes, loop_codes, values) with values = unique(ew).  Repeated edges and more than 65 535
    distinct weights raise ValueError."""
    n = int(n)
    ei = np.ascontiguousarray(ei, np.int64)
    ej = np.ascontiguousarray(ej, np.int64)
    ew = np.ascontiguousarray(ew, np.float64)
    if not (len(ei) == len(ej) == len(ew)):
        raise ValueError("edge arrays differ in length")
    if len(ei) and (min(ei.min(), ej.min()) < 0 or max(ei.max(), ej.max()) >= n):
        raise ValueError("edge endpoint out of range")
    if not np.isfinite(ew).all():
        raise ValueError("edge weights must be finite")
    if (ew < 0).any():
        raise ValueError("edge weights must not be negative")
    values, code = np.unique(ew, return_inverse=True)
    if len(values) > 65535:
        raise ValueError("more than 65535 distinct edge weights")
    lo, hi = np.minimum(ei, ej), np.maximum(ei, ej)
    if len(np.unique(lo * max(n, 1) + hi)) != len(lo):
        raise ValueError("repeated edge")
    d = lo == hi
    loops = np.full(n, 0xFFFF, np.uint16)
    loops[lo[d]] = code[d]
    a = np.concatenate([lo[~d], hi[~d]])
    b = np.concatenate([hi[~d], lo[~d]])
    c = np.concatenate([code[~d], code[~d]])
    o = np.lexsort((b, a))
    ptr = np.zeros(n + 1, np.int64)
    np.add.at(ptr, a + 1, 1)
    return np.cumsum(ptr), b[o].astype(np.int32), c[o].astype(np.uint16), loops, values


def louvain_device(n, ei, ej, ew, resolution=1.05, seed=0, weights=True, return_modularity=False):
    """`louvain_sync_dense` on the GPU (da_dev_louvain_csr), in the ``cluster_fn`` calling convention: the canonical CSR is built here in
    numpy (values = unique(ew)), uploaded, and clustered by `device.louvain_csr`.  Raises ValueError above 65 535 distinct weights, on
    repeated edges, and -- like `louvain_sync_dense` -- on non-finite or negative weights and endpoints out of range."""
    import torch
    from . import device
    ptr, adj, codes, loops, values = canonical_csr(n, ei, ej, ew)
    up = lambda a, t: torch.from_numpy(a.view(t) if a.dtype != t else a).cuda()           # noqa: E731
    member, q, _, _ = device.louvain_csr(up(ptr, np.int64), up(adj, np.int32), up(codes, np.int16), up(loops, np.int16), values,
                                         resolution=resolution, seed=seed, weights=weights)
    return (member, q) if return_modularity else member


# ---- connected components: the definition (numpy), the host call and the device call that reproduce it element for element ------------------
def _cc_edge_arrays(n, ei, ej):
    n = int(n)
    ei = np.ascontiguousarray(ei, np.int64).ravel()
    ej = np.ascontiguousarray(ej, np.int64).ravel()
    if len(ei) != len(ej):
        raise ValueError("edge arrays differ in length")
    if n < 0:
        raise ValueError("n must not be negative")
    if len(ei) and (min(ei.min(), ej.min()) < 0 or max(ei.max(), ej.max()) >= n):
        raise ValueError("edge endpoint out of range")
    return n, ei, ej


def components_dense(n, ei, ej):
    """The connected components of the undirected graph on the vertices 0 .. n - 1 with the edges (ei[e], ej[e]), as their definition in
    numpy: what `components` (host), `components_device` and ``device.components_*`` / ``device.lsh_components`` reproduce element for
    element.  Edges come in any order and either orientation; repeats and self-loops are harmless; endpoints outside [0, n) raise
    ValueError; a vertex without an edge is its own component.

    Returns ``(membership int32[n], n_components)``: with min C(v) the smallest vertex of v's component,
    ``membership[v] = 1 + |{component minima smaller than min C(v)}|`` -- ids from 1 in order of first appearance.  Sizes are
    ``np.bincount(membership)[1:]``.  n = 0 gives an empty array and 0.

    The minimum is found by propagation: label[v] starts as v and every round takes, over all edges, the smaller label of the two ends and
    then jumps label[v] <- label[label[v]] until nothing changes."""
    n, ei, ej = _cc_edge_arrays(n, ei, ej)
    label = np.arange(n, dtype=np.int64)
    while True:
        before = label.copy()
        low = np.minimum(label[ei], label[ej])
        np.minimum.at(label, ei, low)
        np.minimum.at(label, ej, low)
        while True:
            jumped = label[label]
            if np.array_equal(jumped, label):
                break
            label = jumped
        if np.array_equal(before, label):
            break
    is_min = label == np.arange(n, dtype=np.int64)             # label[v] = min C(v)
    rank = np.cumsum(is_min)                                   # 1 + the minima below, at a minimum
    return rank[label].astype(np.int32), int(is_min.sum())


def components(n, ei, ej, ew=None, seed=0, weights=True, return_count=False):
    """`components_dense` through the library's host union-find (da_components; needs no GPU), in the ``cluster_fn`` calling convention:
    ``clusterbreak(..., cluster_fn=components)`` is single-linkage splitting under the recursion's tightening quantile.  Weights and seed
    are ignored.  Returns the membership, with return_count ``(membership, n_components)``.  An endpoint outside [0, n) raises
    DynaAlignError (DA_ERR_BAD_ARG)."""
    lib = _capi.load()
    ei = np.ascontiguousarray(ei, np.int32).ravel()
    ej = np.ascontiguousarray(ej, np.int32).ravel()
    if len(ei) != len(ej):
        raise ValueError("edge arrays differ in length")
    member = np.zeros(max(int(n), 1), np.int32)
    count = np.zeros(1, np.int64)
    _capi.check(lib.da_components(int(n), len(ei), ei.ctypes.data, ej.ctypes.data, member.ctypes.data, count.ctypes.data))
    member = member[:max(int(n), 0)]
    return (member, int(count[0])) if return_count else member


def components_device(n, ei, ej, ew=None, seed=0, weights=True, return_count=False):
    """`components_dense` on the GPU (da_dev_components_edges), in the ``cluster_fn`` calling convention: the edge arrays are uploaded as
    they are -- no canonical form is needed -- and `device.components_edges` labels them.  Weights and seed are ignored.  Like
    `components_dense`, endpoints out of range raise ValueError (checked here, before the upload)."""
    import torch
    from . import device
    n, ei, ej = _cc_edge_arrays(n, ei, ej)
    up = lambda a: torch.from_numpy(a.astype(np.int32)).cuda()                              # noqa: E731
    member, count = device.components_edges(up(ei), up(ej), n)
    return (member, count) if return_count else member


def _quantile_type7_sorted_parts(x, p):
    """stats::quantile(x, p, type = 7) for one probability, R's own arithmetic (quantile.default):
    index = 1 + (n - 1) p; lo = floor, hi = ceiling; qs = x[lo]; if index > lo and x[hi] != qs:
    qs = (1 - h) qs + h x[hi], h = index - lo."""
    n = x.size
    if n == 0:
        return float("nan")                    # quantile(numeric(0), p) is NA
    if np.isnan(x).any():
        raise ValueError("missing values and NaN's not allowed if 'na.rm' is FALSE")
    index = 1.0 + (n - 1) * float(p)
    lo, hi = int(np.floor(index)), int(np.ceil(index))
    part = np.partition(x, sorted({lo - 1, hi - 1}))
    qs, xh = float(part[lo - 1]), float(part[hi - 1])
    if index > lo and xh != qs:
        h = index - lo
        qs = (1.0 - h) * qs + h * xh
    return qs


def threshold_edges_dense(sim, thresh_p):
    """R/clusterbreak.R:219-221 + the graph netcluster builds (:122-124), from a dense matrix:
    threshold = quantile(S[upper.tri(S)], thresh_p); S[S < threshold] <- 0; edges = non-zero entries of the upper
    triangle INCLUDING the diagonal (graph_from_adjacency_matrix(mode = "upper", weighted = TRUE): a zero weight is
    no edge).  Returns (threshold, i, j, weight), i <= j, 0-based, sorted by (i, j)."""
    S = np.array(sim, np.float64)              # a copy: the reference modifies its local pep.sim
    if S.ndim != 2 or S.shape[0] != S.shape[1]:
        raise ValueError("Input must be a square pairwise similarity matrix")          # netcluster, :118-120
    n = S.shape[0]
    upper = np.triu(np.ones((n, n), bool), 1)                                          # upper.tri(pep.sim)
    thr = _quantile_type7_sorted_parts(S[upper], thresh_p)
    del upper
    if not np.isnan(thr):
        S[S < thr] = 0.0
    U = np.triu(S)                                                                     # mode = "upper": diagonal included
    i, j = np.nonzero(U)                                                               # row-major = sorted by (i, j)
    return thr, i.astype(np.int32), j.astype(np.int32), U[i, j]


def netcluster(pepmat, igraph_mode="upper", igraph_weight=True, cluster_func=None, cluster_weight=True, seed=0):
    """reference netcluster (R/clusterbreak.R:112-136) on a dense matrix: graph from the upper triangle incl. the
    diagonal, then cluster_func(n, i, j, w, seed=..., weights=...) -> numeric vector of cluster ids."""
    M = np.asarray(pepmat, np.float64)
    if M.ndim != 2 or M.shape[0] != M.shape[1]:
        raise ValueError("Input must be a square pairwise similarity matrix")
    n = M.shape[0]
    i, j = np.triu_indices(n, 0)
    # igraph::graph_from_adjacency_matrix(mode = ...) for the undirected modes (igraph's documentation; igraph itself is not
    # importable here, so everything but "upper" -- the reference's default and the only mode clusterbreak uses -- is unpinned)
    if igraph_mode == "upper":
        w = M[i, j]
    elif igraph_mode == "lower":
        w = M[j, i]
    elif igraph_mode in ("max", "undirected"):
        w = np.maximum(M[i, j], M[j, i])
    elif igraph_mode == "min":
        w = np.minimum(M[i, j], M[j, i])
    elif igraph_mode == "plus":
        w = np.where(i == j, M[i, j], M[i, j] + M[j, i])
    elif igraph_mode == "directed":
        raise ValueError("igraph_mode = 'directed' builds a directed graph; igraph::cluster_louvain only works with undirected graphs")
    else:
        raise ValueError("igraph_mode must be one of 'upper', 'lower', 'max', 'undirected', 'min', 'plus'")
    nz = w != 0.0
    i, j, w = i[nz].astype(np.int32), j[nz].astype(np.int32), w[nz]
    if not igraph_weight:
        w = np.ones_like(w)
    return _run_cluster_fn(cluster_func or louvain, n, i, j, w, cluster_weight, seed)


def _run_cluster_fn(cluster_fn, n, i, j, w, cluster_wt, seed):
    # netcluster (R/clusterbreak.R:125-129) calls cluster_func(network, weights = E(network)$weight) or cluster_func(network).
    # For the default cluster_func the second form is NOT unweighted: igraph::cluster_louvain(weights = NULL) takes the graph's
    # `weight` edge attribute when there is one, and graph_from_adjacency_matrix(weighted = TRUE) always creates it -- so the
    # built-in Louvain keeps the weights whatever cluster_wt says (an unweighted graph arrives here with w = 1).  A caller's own
    # cluster_fn sees the flag, as the reference's sees the presence of the `weights` argument.
    builtin = cluster_fn is louvain
    out = cluster_fn(n, i, j, w, seed=seed, weights=True if builtin else bool(cluster_wt))
    out = np.asarray(out)
    if out.ndim != 1 or out.size != n or not np.issubdtype(out.dtype, np.number):
        raise ValueError("Wrong clustering output format. Output should be a numeric vector of cluster assignment.")  # :134
    return out.astype(np.int64)


def _csr_to_edges(ptr, adj, codes, loops, values):
    """the symmetric CSR of MinHashSession.edges_csr / knn_csr as the edge list (i <= j, weight) sorted by (i, j), self-loops included"""
    n = len(ptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
    up = adj > rows
    ei, ej, ew = rows[up], adj[up].astype(np.int64), values[codes[up]]
    has = np.nonzero(loops != 0xFFFF)[0]
    ei, ej, ew = np.concatenate([ei, has]), np.concatenate([ej, has]), np.concatenate([ew, values[loops[has]]])
    order = np.lexsort((ej, ei))
    return ei[order].astype(np.int32), ej[order].astype(np.int32), ew[order]


class ClusterbreakResult(dict):
    """list(clustered_seq = <n x 2: sequence, "<itr>.<cluster>">, filtered_seq = <sequences>) of the reference
    (R/clusterbreak.R:257-258), plus bookkeeping the reference only prints: .convergence (1 / 0, :200,:213),
    .calls (state$itr, :270), .levels (per call: itr, n, threshold, edges, clusters, seconds by phase)."""


def clusterbreak(pep, thresh_p=0.8, size_max=10, size_min=3, max_itr=10000, sim_fn=None, cluster_fn=None,
                 cluster_wt=True, *, session=None, edges_fn=None, cluster_seed=0, verbose=False, log=None, knn=None, knn_mode="union",
                 knn_lsh=None, louvain="host", louvain_device_min_nnz=LOUVAIN_DEVICE_MIN_NNZ):
    """Recursive quantile-threshold + Louvain splitting, reference clusterbreak (R/clusterbreak.R:180-275).

    pep        sequences (character vector)
    sim_fn     sequences -> similarity matrix; default = the reference's default, similarityMH(x, k=2, n_hash=50)
    session    a MinHashSession over `pep`: levels then run on the device edge path and sim_fn is not used
    edges_fn   sequences -> (threshold, i, j, weight), the thresholded graph of a level as an edge list (i <= j, the diagonal included,
               0-based): called on every level's sequences in place of sim_fn + threshold_edges_dense, e.g.
               ``lambda s: similarityNW_edges_long(s, thresh_p=0.8)``; a level of fewer than 2 sequences does not call it
    cluster_fn (n, i, j, w, seed=, weights=) -> ids; default `louvain` with resolution 1.05
    knn        with a session: a level of m >= 2 sequences clusters on the kNN graph session.knn_csr(idx, min(knn, m - 1), knn_mode) -- at most
               m * knn edges in place of the quantile's fixed share of m^2 (thresh_p is not used); knn_mode "union" or "mutual".  Without a
               session give the graph as ``edges_fn=lambda s: similarityMH_knn_edges(s, k, n_hash, top, mode)``.  The memberships are not
               those of the quantile threshold: it is another graph.  None (default): the quantile threshold
    knn_lsh    with a session and knn: a (bands, rows) pair -- a level takes its kNN graph from LSH candidates,
               session.lsh_knn_csr(bands, rows, idx, min(knn, m - 1), knn_mode), in place of session.knn_csr: only bucket mates are compared,
               and a neighbour that agrees in no whole band is missing.  Without a session give the graph as
               ``edges_fn=lambda s: similarityMH_lsh_knn_edges(s, k, n_hash, bands, rows, top, mode)``.  None (default): all pairs
    cluster_seed  call number c of the recursion clusters with seed cluster_seed + c (the reference draws from
               R's global RNG instead)
    louvain    "host" (default): the built-in `louvain_csr`.  "device" (needs a session and no cluster_fn): a level whose CSR has at least
               louvain_device_min_nnz adjacency entries is clustered where it lies, by `device.louvain_csr` -- the synchronous Louvain
               `louvain_sync_dense` defines, with seed cluster_seed + c -- and the graph is not copied to the host; smaller levels take the
               host path.  The memberships are not the host Louvain's: it is another clustering function
    """
    if size_max <= size_min:
        raise ValueError("size_max must be greater than size_min")                      # :189-191
    pep = list(pep)
    if len(pep) == 0:
        raise ValueError("empty input sequence vector")                                  # :192-194
    if session is not None and session.n != len(pep):
        raise ValueError("session holds %d sequences, pep has %d" % (session.n, len(pep)))
    if edges_fn is not None and session is not None:
        raise ValueError("edges_fn and session both produce a level's edge list: give one of them")
    if knn is not None:
        if session is None:
            raise ValueError("knn needs a session; without one give the kNN graph as edges_fn=lambda s: similarityMH_knn_edges(s, k, n_hash, top, mode)")
        if knn_mode not in ("union", "mutual"):
            raise ValueError("knn_mode must be 'union' or 'mutual'")
        knn = int(knn)
        if knn < 1:
            raise ValueError("knn must be at least 1")
    if knn_lsh is not None:
        if session is None or knn is None:
            raise ValueError("knn_lsh needs a session and knn; without them give the graph as "
                             "edges_fn=lambda s: similarityMH_lsh_knn_edges(s, k, n_hash, bands, rows, top, mode)")
        try:
            lsh_bands, lsh_rows = (int(v) for v in knn_lsh)
        except (TypeError, ValueError):
            raise ValueError("knn_lsh must be a (bands, rows) pair") from None

    import os
    if louvain not in ("host", "device"):
        raise ValueError("louvain must be 'host' or 'device'")
    if louvain == "device" and (session is None or cluster_fn is not None):
        raise ValueError("louvain='device' clusters the session's resident CSR: it needs a session and no cluster_fn")
    on_dev = louvain == "device"
    if on_dev and os.environ.get("DYNAALIGN_CLUSTERBREAK_NO_CSR"):
        raise ValueError("louvain='device' clusters the CSR path's graph: unset DYNAALIGN_CLUSTERBREAK_NO_CSR")

    def knn_csr(idx, m):
        if knn_lsh is not None:
            return (session.lsh_knn_csr_device if on_dev else session.lsh_knn_csr)(lsh_bands, lsh_rows, idx, min(knn, m - 1), knn_mode)
        return (session.knn_csr_device if on_dev else session.knn_csr)(idx, min(knn, m - 1), knn_mode)
    if sim_fn is None and session is None and edges_fn is None:
        from .similarity import similarityMH
        sim_fn = lambda x: similarityMH(x, k=2, n_hash=50)                               # noqa: E731  (:185)
    csr_path = session is not None and cluster_fn is None and not os.environ.get("DYNAALIGN_CLUSTERBREAK_NO_CSR")
    cluster_fn = cluster_fn or _louvain_host           # (`louvain` is this function's mode argument)
    out_seq, out_lab, filtered = [], [], []                                              # state$out.df, state$filter.df
    state = {"itr": 1, "convergence": 1}                                                 # :199-200
    levels = []

    def log_message(msg, level="INFO"):                                                  # :206-209
        if verbose or level != "INFO":
            print("[%s] %s: %s" % (time.strftime("%H:%M:%S"), level, msg), file=log or sys.stdout)

    def level_edges(idx):
        m = len(idx)
        if session is not None or edges_fn is not None:
            if m < 2:                          # quantile(numeric(0)) is NA: nothing is removed, the 1.0 diagonal stays
                return float("nan"), np.zeros(m, np.int32), np.zeros(m, np.int32), np.ones(m, np.float64)
            if edges_fn is not None:
                thr, ei, ej, ew = edges_fn([pep[t] for t in idx])
                return float(thr), np.asarray(ei, np.int32), np.asarray(ej, np.int32), np.asarray(ew, np.float64)
            if knn is not None:
                thr, _, ptr, adj, codes, loops, values = knn_csr(idx, m)
                return (thr,) + _csr_to_edges(ptr, adj, codes, loops, values)
            return session.edges(idx, thresh_p, sort=False)
        return threshold_edges_dense(sim_fn([pep[t] for t in idx]), thresh_p)

    def cluster_recursive(idx):
        if state["itr"] > max_itr:                                                       # :211-215
            log_message("Maximum function calls reached", "WARNING")
            state["convergence"] = 0
            return
        itr = state["itr"]
        t0 = time.perf_counter()
        m = len(idx)
        seed_c = (int(cluster_seed) + itr) & 0xFFFFFFFF
        if csr_path and m >= 2:
            # device edge path + built-in Louvain: the graph arrives as canonical CSR sorted on the device (same graph, same result)
            if knn is not None:
                thr, n_edges, ptr, adj, codes, loops, values = knn_csr(idx, m)
            else:
                thr, n_edges, ptr, adj, codes, loops, values = session.edges_csr(idx, thresh_p, **({"on_device": True} if on_dev else {}))
            if on_dev:               # the graph kernels are asynchronous: their time belongs to similarity_s, not to cluster_s
                import torch
                torch.cuda.synchronize()
            t1 = time.perf_counter()
            if on_dev and int(adj.numel()) >= int(louvain_device_min_nnz):
                from . import device
                c_index = device.louvain_csr(ptr, adj, codes, loops, values, seed=seed_c, weights=True)[0].astype(np.int64)
            else:
                if on_dev:           # a small level: launch-bound on the device, so the host Louvain takes it
                    ptr, adj = ptr.cpu().numpy(), adj.cpu().numpy()
                    codes, loops = codes.cpu().numpy().view(np.uint16), loops.cpu().numpy().view(np.uint16)
                c_index = louvain_csr(m, ptr, adj, codes, loops, values, seed=seed_c, weights=True).astype(np.int64)   # :222 (built-in: see _run_cluster_fn)
            del ptr, adj, codes, loops
        else:
            thr, ei, ej, ew = level_edges(idx)
            n_edges = len(ei)
            t1 = time.perf_counter()
            c_index = _run_cluster_fn(cluster_fn, m, ei, ej, ew, cluster_wt, seed_c)     # :222
            del ei, ej, ew
        t2 = time.perf_counter()
        c_size = np.bincount(c_index, minlength=1)[1:] if m else np.zeros(0, np.int64)   # tabulate(c.index)   :224
        ids = np.arange(1, len(c_size) + 1)
        id_itr = ids[c_size > size_max]                                                  # :225
        id_rm = ids[c_size < size_min]                                                   # :226
        in_rm = np.isin(c_index, id_rm)
        in_itr = np.isin(c_index, id_itr)
        filtered.extend(pep[idx[t]] for t in np.nonzero(in_rm)[0])                       # :228
        keep = ~in_rm & ~in_itr                                                          # :232 / :238 (in_itr is empty in the first case)
        nkeep = int(keep.sum())
        if nkeep == 1:
            # pep.ref[mask, ] with one TRUE row drops to a character vector, nrow() is NULL and `if (NULL > 0)` stops
            raise RuntimeError("argument is of length zero")
        for t in np.nonzero(keep)[0]:                                                    # :233-236 / :239-243
            out_seq.append(pep[idx[t]])
            out_lab.append("%d.%d" % (itr, c_index[t]))
        levels.append({"itr": itr, "n": m, "threshold": thr, "edges": int(n_edges), "clusters": int(len(c_size)),
                       "oversize": int(len(id_itr)), "similarity_s": t1 - t0, "cluster_s": t2 - t1})
        log_message("call %d: n=%d threshold=%g edges=%d clusters=%d oversize=%d (similarity %.3f s, clustering %.3f s)"
                    % (itr, m, thr, n_edges, len(c_size), len(id_itr), t1 - t0, t2 - t1))
        if len(id_itr) == 0:
            return
        # :246-254 -- oversize clusters in order of first appearance (unique(pep.new[,2])), each a new call
        sub = c_index[in_itr]
        _, first = np.unique(sub, return_index=True)
        for cid in sub[np.sort(first)]:
            state["itr"] += 1                                                            # :252
            cluster_recursive(idx[c_index == cid])                                       # :251,:253

    cluster_recursive(np.arange(len(pep), dtype=np.int64))
    if verbose:                                                                          # :265-270
        print("\nClustering complete:" if state["convergence"] == 1 else "\nClustering incomplete, consider adjusting parameters:",
              file=log or sys.stdout)
        print("Total function calls (clusters broken): %d" % state["itr"], file=log or sys.stdout)
    res = ClusterbreakResult(clustered_seq=np.array(list(zip(out_seq, out_lab)), dtype=object).reshape(-1, 2),
                             filtered_seq=filtered)
    res.convergence, res.calls, res.levels = state["convergence"], state["itr"], levels
    return res


CONSENSUS_SYMBOLS = "ARNDCQEGHILKMFPSTWYVBZX*-"   # tie order of clusterconsensus among symbols other than the center's


def clusterconsensus(df, *, matrixName="BLOSUM62", gapOpen=10, gapExt=4, align_fn=None):
    """One consensus sequence per cluster: the reference's signature (R/clusterbreak.R:309-320), ``df`` being rows of
    ``(sequence, cluster_id)`` -- e.g. ``clusterbreak(...)["clustered_seq"]`` -- and the result a list of ``(cluster_id, consensus)`` in
    first-appearance order of the ids.

    This is a CENTER-STAR consensus on the library's own alignments (``nw_align``), NOT DECIPHER's AlignSeqs + ConsensusSequence, which
    the reference calls and which is not restated here; the strings differ from the reference's in general.  For a cluster with members
    s_0 .. s_{c-1} (input order, duplicates kept):

      * c == 1: the member itself;
      * the center is the member i with the largest ``math.fsum(matches[i, j] / length[i, j] for j != i)`` of the alignments of s_i
        as sequence1 with s_j (a pair of two empty strings counts 0.0), ties to the lowest i -- one ``nw_align(ops=False)`` call over all
        ordered pairs of all clusters;
      * a second call aligns every center, as sequence1, with the other members of its cluster.  For center position p the tally holds
        the center's residue and, per other member, the residue a D step puts opposite p, or '-' for a U step; L steps (residues
        inserted between center positions) are ignored;
      * the most frequent symbol wins; among tied symbols the center's residue if it is one of them, otherwise the one earliest in
        "ARNDCQEGHILKMFPSTWYVBZX*-"; positions won by '-' are dropped.

    ``align_fn`` (a hook in the style of ``clusterbreak``'s ``sim_fn`` / ``cluster_fn``): the alignment call, ``None`` for ``nw_align``.
    It is called twice as ``align_fn(pool, pool, matrixName, gapOpen, gapExt, pairs=(pi, pj), ops=bool)`` and returns what ``nw_align``
    returns.  With the default, sequences longer than 127 residues raise the library's error (DA_ERR_UNSUPPORTED);
    ``align_fn=nw_align_long`` takes sequences of up to 1024 residues."""
    import math
    if align_fn is None:
        from .similarity import nw_align as align_fn
    rows = df["clustered_seq"] if isinstance(df, dict) else df
    order, members = [], {}
    for row in rows:
        seq, cid = row[0], row[1]
        seq = seq.decode("latin-1") if isinstance(seq, bytes) else str(seq)
        if cid not in members:
            members[cid] = []
            order.append(cid)
        members[cid].append(seq)
    # every member of a cluster of two or more, pooled: both calls index this one list
    pool, start = [], {}
    for cid in order:
        if len(members[cid]) > 1:
            start[cid] = len(pool)
            pool.extend(members[cid])
    center = {}
    if pool:
        pi, pj = [], []
        for cid in start:
            b, c = start[cid], len(members[cid])
            for i in range(c):
                for j in range(c):
                    if i != j:
                        pi.append(b + i)
                        pj.append(b + j)
        r = align_fn(pool, pool, matrixName, gapOpen, gapExt, pairs=(pi, pj), ops=False)
        at = 0
        for cid in start:
            c = len(members[cid])
            best, best_sum = 0, None
            for i in range(c):
                tot = math.fsum((int(r.matches[t]) / int(r.length[t])) if r.length[t] else 0.0 for t in range(at, at + c - 1))
                at += c - 1
                if best_sum is None or tot > best_sum:
                    best, best_sum = i, tot
            center[cid] = best
        pi, pj = [], []
        for cid in start:
            b, c = start[cid], len(members[cid])
            for j in range(c):
                if j != center[cid]:
                    pi.append(b + center[cid])
                    pj.append(b + j)
        r = align_fn(pool, pool, matrixName, gapOpen, gapExt, pairs=(pi, pj), ops=True)
    out, at = [], 0
    for cid in order:
        mem = members[cid]
        if len(mem) == 1:
            out.append((cid, mem[0]))
            continue
        cen = mem[center[cid]]
        tally = [{ch: 1} for ch in cen]
        for j in range(len(mem)):
            if j == center[cid]:
                continue
            other, ops = mem[j], r.ops[at]
            at += 1
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
        cons = []
        for p, t in enumerate(tally):
            top = max(t.values())
            tied = [ch for ch in t if t[ch] == top]
            win = cen[p] if cen[p] in tied else min(tied, key=CONSENSUS_SYMBOLS.index)
            if win != "-":
                cons.append(win)
        out.append((cid, "".join(cons)))
    return out


def clusterconsensus_device(df, *, matrixName="BLOSUM62", gapOpen=10, gapExt=4, return_centers=False):
    """``clusterconsensus`` with both of its phases on the device (da_cluster_consensus): the same CENTER-STAR consensus, by definition the
    result of ``clusterconsensus(df, align_fn=nw_align_long)`` -- the same list of ``(cluster_id, consensus)``, the same strings, the same
    errors -- and, for sequences of up to 127 residues, of ``clusterconsensus(df)``.  ``df`` as there: rows of ``(sequence, cluster_id)``,
    an object array, or a ``clusterbreak`` result.

    Nothing is listed or summed on the host: the kernels of consensus_kernels.hip list the ordered in-cluster pairs for the alignment
    kernels, add every member's ``matches / length`` terms exactly (63-bit fixed point in two 64-bit limbs) and round the sum to a
    double as ``math.fsum`` does before choosing the center, then tally the centers' alignments column by column and apply the tie rule
    of ``clusterconsensus``.  Clusters of one are copied through on the host, unvalidated; if every cluster has one member no device
    is needed.  Members of clusters of two or more have 0 .. 1024 residues.

    ``return_centers=True``: returns ``(consensus_list, centers)``, ``centers[t]`` the index into the rows of the center of the t-th
    cluster (of its only member for a cluster of one)."""
    from .similarity import _as_int, _matrix_name, pack_sequences
    rows = df["clustered_seq"] if isinstance(df, dict) else df
    order, members, where = [], {}, {}
    for at, row in enumerate(rows):
        seq, cid = row[0], row[1]
        seq = seq.decode("latin-1") if isinstance(seq, bytes) else str(seq)
        if cid not in members:
            members[cid] = []
            where[cid] = []
            order.append(cid)
        members[cid].append(seq)
        where[cid].append(at)
    # every member of a cluster of two or more, pooled; the library numbers these clusters 0, 1, ... in first-appearance order
    pooled = [cid for cid in order if len(members[cid]) > 1]
    cons, center = {}, {}
    if pooled:
        pool, index, cluster_of = [], [], []
        for k, cid in enumerate(pooled):
            pool.extend(members[cid])
            index.extend(where[cid])
            cluster_of.extend([k] * len(members[cid]))
        lib = _capi.load()
        res, off = pack_sequences(pool)
        cl = np.asarray(cluster_of, np.int32)
        ld = max(int(np.diff(off).max()), 1)
        out = np.zeros((len(pooled), ld), np.uint8)
        out_len = np.zeros(len(pooled), np.int32)
        out_center = np.zeros(len(pooled), np.int32)
        name = _matrix_name(matrixName)
        _capi.check(lib.da_cluster_consensus(res.ctypes.data, off.ctypes.data, len(pool), cl.ctypes.data, len(pooled), name,
                                             _as_int(gapOpen, "gapOpen"), _as_int(gapExt, "gapExt"), out.ctypes.data, ld, out_len.ctypes.data,
                                             out_center.ctypes.data))
        raw = out.tobytes()
        for k, cid in enumerate(pooled):
            cons[cid] = raw[k * ld:k * ld + int(out_len[k])].decode("latin-1")
            center[cid] = index[int(out_center[k])]
    result = [(cid, cons[cid] if cid in cons else members[cid][0]) for cid in order]
    if return_centers:
        return result, [center[cid] if cid in center else where[cid][0] for cid in order]
    return result
