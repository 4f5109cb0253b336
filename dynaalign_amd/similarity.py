"""Host-side mirror of the reference's R interface for the hot path.

    similarityMH(sequences, k=4, n_hash=50)                      reference R/RcppExports.R:15-17
    similarityNW(sequences, matrixName="BLOSUM62", gapOpen=10, gapExt=4)   reference R/RcppExports.R:34-36

and their two-set forms (no counterpart in the reference: a second set against the first, an m x n matrix)

    similarityMH_cross(x, y, k=4, n_hash=50)
    similarityNW_cross(x, y, matrixName="BLOSUM62", gapOpen=10, gapExt=4)

and the top-k forms of those (per row of x the ``top`` most similar y, never the m x n matrix)

    similarityMH_cross_topk(x, y, k=4, n_hash=50, top=10)
    similarityNW_cross_topk(x, y, matrixName="BLOSUM62", gapOpen=10, gapExt=4, top=10)

and the top-k form of ONE set against itself (per sequence its ``top`` most similar other sequences, and the kNN graph of those lists)

    similarityMH_knn(sequences, k=4, n_hash=50, top=10)            similarityMH_knn_edges(..., top=10, mode="union")
    similarityNW_knn(sequences, matrixName="BLOSUM62", gapOpen=10, gapExt=4, top=10)     similarityNW_knn_edges(..., top=10, mode="union")
    similarityNW_knn_long(...), similarityNW_knn_edges_long(...), similarityNW_cross_topk_long(...)    the same for 1 .. 1024 residues
    knn_dense(S, top), knn_graph(idx, val, diag=None, mode="union")   the definitions in numpy

and the EXACT Jaccard index of the k-shingle sets that similarityMH estimates (sequences of at most 127 shingles, k <= 8; no hash functions, no seed)

    similarityJaccard(sequences, k=4)                    similarityJaccard_cross(x, y, k=4)
    similarityJaccard_cross_topk(x, y, k=4, top=10)      similarityJaccard_knn(sequences, k=4, top=10)
    similarityJaccard_knn_edges(sequences, k=4, top=10, mode="union")      similarityJaccard_edges(sequences, k=4, thresh_p=0.8)
    jaccard_dense(sequences, k, y=None), jaccard_counts(sequences, k, y=None)   the definition in Python
    similarityJaccard_long(...), _cross_long, _cross_topk_long, _knn_long, _knn_edges_long, _edges_long, _stats_long: the same for up to 1024
    shingles, and similarityJaccard_cross_edges_long(x, y, k=4, thresh_p=0.8, threshold=None), the two-set threshold form

and the Levenshtein similarity (L - d) / L of plain edit distance d, L the longer length (sequences of at most 127 bytes, any byte values)

    similarityLev(sequences)                             similarityLev_cross(x, y)
    similarityLev_cross_topk(x, y, top=10)               similarityLev_knn(sequences, top=10)
    similarityLev_knn_edges(sequences, top=10, mode="union")               similarityLev_edges(sequences, thresh_p=0.8)
    similarityLev_cross_edges(x, y, thresh_p=0.8, threshold=None)          the range query: "everything within t edits"
    lev_dense(sequences, y=None), lev_counts(sequences, y=None)            the definition in Python

and the threshold forms of those (the entries that pass a threshold as a sorted edge list, never the m x n matrix)

    similarityMH_cross_edges(x, y, k=4, n_hash=50, thresh_p=0.8, threshold=None)
    similarityNW_cross_edges(x, y, matrixName="BLOSUM62", gapOpen=10, gapExt=4, thresh_p=0.8, threshold=None)

and the NW threshold forms for sequences of up to 1024 residues (32-bit value ranks on the device in place of the uint16 code)

    similarityNW_edges_long(sequences, matrixName="BLOSUM62", gapOpen=10, gapExt=4, thresh_p=0.8)
    similarityNW_cross_edges_long(x, y, matrixName="BLOSUM62", gapOpen=10, gapExt=4, thresh_p=0.8, threshold=None)

and the alignment itself for listed pairs (which residue sits opposite which: the path the reference's traceback walks)

    nw_align(x, y, matrixName="BLOSUM62", gapOpen=10, gapExt=4, pairs=None, ops=True)
    nw_align_long(x, y, matrixName="BLOSUM62", gapOpen=10, gapExt=4, pairs=None, ops=True)

Same names, argument order, defaults and error texts as the reference; the
bodies marshal to the C ABI (include/dynaalign.h) exactly as the Rcpp glue in
r_glue/ does.  Results are dense symmetric n x n float64 matrices with
``dimnames`` ("1".."n", reference src/minHash.cpp:181-185,
src/pairwiseSeqAlign.cpp:356-362).

Seeds: the reference draws its hash seeds from ``std::random_device``
(src/minHash.cpp:73,137), so it is non-deterministic by construction.  The
default here does the same.  For reproducible runs set ``seed=`` (keyword-only
extension), ``set_option("seed", s)`` or the environment variable
``DYNAALIGN_SEED``; the seed is expanded with the reference's own rule
(``HashFamily(n_hash, seed)``, src/minHash.cpp:73-81).
"""
import ctypes
import os

import numpy as np

from . import _capi

# options(DynaAlign.seed = , DynaAlign.devices = , DynaAlign.exchange = ) of the R glue (r_glue/)
_OPTIONS = {"seed": None, "devices": None, "exchange": "rows"}


def set_option(name, value):
    if name not in _OPTIONS:
        raise KeyError(name)
    _OPTIONS[name] = value


def get_option(name):
    return _OPTIONS[name]


class SimilarityMatrix(np.ndarray):
    """float64 (n, n) ndarray -- (m, n) for the two-set calls -- carrying R-style ``dimnames``."""

    def __new__(cls, arr):
        obj = np.asarray(arr).view(cls)
        n = obj.shape[0]
        labels = [str(i + 1) for i in range(n)]
        obj.dimnames = [labels, [str(j + 1) for j in range(obj.shape[1])] if obj.ndim == 2 else list(labels)]
        return obj

    def __array_finalize__(self, obj):
        self.dimnames = getattr(obj, "dimnames", None)


def pack_sequences(sequences):
    """Character vector -> (residues uint8[total], offsets int64[n+1]).

    Bytes are taken as they are (no case folding, no re-encoding), like
    ``as<std::string>`` on a CHARSXP (reference src/minHash.cpp:147)."""
    if isinstance(sequences, (str, bytes)):
        sequences = [sequences]
    bs = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in sequences]
    off = np.zeros(len(bs) + 1, np.int64)
    if bs:
        np.cumsum([len(b) for b in bs], out=off[1:])
    total = int(off[-1])
    res = np.frombuffer(b"".join(bs), np.uint8).copy() if total else np.zeros(1, np.uint8)
    return res, off


def _as_int(x, name):
    # R coerces numeric to int at the .Call boundary (Rcpp input_parameter<int>)
    try:
        return int(x)
    except Exception:
        raise TypeError("%s must be an integer" % name)


def _matrix_name(matrixName):
    return matrixName.encode("latin-1") if isinstance(matrixName, str) else bytes(matrixName)


def _pack_two(x, y):
    """two character vectors -> (x residues, x offsets, m, y residues, y offsets, n)"""
    xr, xo = pack_sequences(x)
    yr, yo = pack_sequences(y)
    return xr, xo, len(xo) - 1, yr, yo, len(yo) - 1


def _topk_arrays(rows, top, limit):
    """-> (top, idx int32, val float64): the host arrays of a top-k call, at least one slot each way, with ``top`` clamped to ``limit``,
    the number of candidates a row has, when there is one (the C ABI does not clamp)"""
    top = _as_int(top, "top")
    if limit >= 1:
        top = min(top, limit)
    shape = (max(rows, 1), max(top, 1))
    return top, np.empty(shape, np.int32), np.empty(shape, np.float64)


def hash_family_seeds(seed, n_hash):
    """seeds[h] = h-th raw std::mt19937(seed) output (reference src/minHash.cpp:75-80)."""
    lib = _capi.load()
    out = np.zeros(max(int(n_hash), 1), np.uint32)
    _capi.check(lib.da_hash_family_seeds(int(seed) & 0xFFFFFFFF, int(n_hash), out.ctypes.data))
    return out[:n_hash]


def _resolve_seed(seed):
    if seed is None:
        seed = _OPTIONS["seed"]
    if seed is None and os.environ.get("DYNAALIGN_SEED"):
        seed = int(os.environ["DYNAALIGN_SEED"])
    if seed is None:
        seed = _capi.load().da_random_seed()  # reference default: std::random_device{}()
    return int(seed) & 0xFFFFFFFF


def _mh_prelude(sequences, k, n_hash, seed):
    lib = _capi.load()
    res, off = pack_sequences(sequences)
    n = len(off) - 1
    k, n_hash = _as_int(k, "k"), _as_int(n_hash, "n_hash")
    # validation (and its order) lives in the library; seeds are only needed when it passes
    seeds = hash_family_seeds(_resolve_seed(seed), n_hash) if n_hash > 0 else np.zeros(1, np.uint32)
    if len(seeds) == 0:
        seeds = np.zeros(1, np.uint32)
    return lib, res, off, n, k, n_hash, seeds


def _mh_prelude_two(x, y, k, n_hash, seed):
    """_mh_prelude on ``x``, then ``y`` packed -> (lib, x residues, x offsets, m, y residues, y offsets, n, k, n_hash, seeds)"""
    lib, xr, xo, m, k, n_hash, seeds = _mh_prelude(x, k, n_hash, seed)
    yr, yo = pack_sequences(y)
    return lib, xr, xo, m, yr, yo, len(yo) - 1, k, n_hash, seeds


def _device_opts(devices, exchange):
    """da_opts for the multi-device entry points, or None for the plain single-device call"""
    devices = _OPTIONS["devices"] if devices is None else devices
    exchange = exchange or _OPTIONS["exchange"] or "rows"
    if devices is None and os.environ.get("DYNAALIGN_DEVICES"):
        devices = [int(d) for d in os.environ["DYNAALIGN_DEVICES"].split(",") if d.strip() != ""]
    if devices is None:
        return None, None
    if isinstance(devices, int):
        devices = [devices]
    return _capi.make_opts(devices, exchange)


last_phase_ms = {}   # phase times of the most recent multi-device call (da_opts.phase_ms), by phase name


def _record_phases(keep):
    last_phase_ms.clear()
    if keep is not None:
        last_phase_ms.update(zip(_capi.DA_PHASES, [float(v) for v in keep[1]]))


def similarityMH(sequences, k=4, n_hash=50, *, seed=None, devices=None, exchange=None):
    """MinHash-estimated Jaccard similarity of k-mer sets, all pairs.

    Mirrors reference ``similarityMH`` (src/minHash.cpp:119-188): errors
    "Input sequences vector cannot be empty" / "'k' must be a positive integer" /
    "Number of hash functions must be positive" in that order; diagonal 1.0.

    devices= / set_option("devices", [...]) / DYNAALIGN_DEVICES=0,1,..: run on several GPUs of the node from this one
    process (da_similarity_mh_opts); exchange = "rows" (default), "allgather" (RCCL) or "peercopy"."""
    lib, res, off, n, k, n_hash, seeds = _mh_prelude(sequences, k, n_hash, seed)
    out = np.empty((max(n, 1), max(n, 1)), np.float64)
    opts, keep = _device_opts(devices, exchange)
    if opts is None:
        _capi.check(lib.da_similarity_mh(res.ctypes.data, off.ctypes.data, n, k, n_hash, seeds.ctypes.data,
                                         out.ctypes.data))
    else:
        _capi.check(lib.da_similarity_mh_opts(res.ctypes.data, off.ctypes.data, n, k, n_hash, seeds.ctypes.data,
                                              out.ctypes.data, ctypes.addressof(opts)))
    _record_phases(keep)
    return SimilarityMatrix(out[:n, :n])


def similarityMH_cross(x, y, k=4, n_hash=50, *, seed=None):
    """MinHash similarity of every sequence of ``x`` against every sequence of ``y``: the (m, n) matrix
    R[i, j] = #{h : sig_x[i, h] == sig_y[j, h]} / n_hash -- bit for bit the block [0:m, m:m+n] of
    ``similarityMH(x + y, k, n_hash)`` under the same seeds.  No forced diagonal: an element is 1.0 only because the
    signatures agree.  Errors as similarityMH, with "Input sequences vector cannot be empty" for ``x``, then for ``y``."""
    lib, xr, xo, m, yr, yo, n, k, n_hash, seeds = _mh_prelude_two(x, y, k, n_hash, seed)
    out = np.empty((max(m, 1), max(n, 1)), np.float64)
    _capi.check(lib.da_similarity_mh_cross(xr.ctypes.data, xo.ctypes.data, m, yr.ctypes.data, yo.ctypes.data, n, k, n_hash,
                                           seeds.ctypes.data, out.ctypes.data, 0))
    return SimilarityMatrix(out[:m, :n])


def similarityMH_cross_topk(x, y, k=4, n_hash=50, top=10, *, seed=None):
    """For every sequence of ``x`` its ``top`` most similar sequences of ``y`` under similarityMH_cross, without the (m, n) matrix:
    returns ``(idx, val)``, (m, top) int32 0-based positions in ``y`` and the (m, top) float64 similarities, with
    ``idx == np.argsort(-R, axis=1, kind="stable")[:, :top]`` and ``val[i, t]`` bit for bit ``R[i, idx[i, t]]`` for
    R = similarityMH_cross(x, y, k, n_hash, seed=seed): value descending, position ascending among equals; columns of
    similarity 0 fill a row with fewer than ``top`` positive ones.  ``top`` is clamped to ``len(y)`` (the C ABI does not clamp) and may be
    at most 1024.  Errors as similarityMH_cross."""
    lib, xr, xo, m, yr, yo, n, k, n_hash, seeds = _mh_prelude_two(x, y, k, n_hash, seed)
    t, idx, val = _topk_arrays(m, top, n)
    _capi.check(lib.da_similarity_mh_cross_topk(xr.ctypes.data, xo.ctypes.data, m, yr.ctypes.data, yo.ctypes.data, n, k, n_hash,
                                                seeds.ctypes.data, t, idx.ctypes.data, val.ctypes.data))
    return idx[:m], val[:m]


def minhash_signatures(sequences, k=4, n_hash=50, *, seed=None):
    """The (n, n_hash) uint32 signature matrix (reference src/minHash.cpp:140-157)."""
    lib, res, off, n, k, n_hash, seeds = _mh_prelude(sequences, k, n_hash, seed)
    out = np.empty((max(n, 1), max(n_hash, 1)), np.uint32)
    _capi.check(lib.da_minhash_signatures(res.ctypes.data, off.ctypes.data, n, k, n_hash, seeds.ctypes.data,
                                          out.ctypes.data))
    return out[:n, :n_hash]


def mh_counts(sequences, k=4, n_hash=50, *, seed=None, row_begin=0, row_end=None):
    """uint16 match counts (numerator at reference src/minHash.cpp:168-174) for a row block."""
    lib, res, off, n, k, n_hash, seeds = _mh_prelude(sequences, k, n_hash, seed)
    row_end = n if row_end is None else row_end
    out = np.empty((max(row_end - row_begin, 1), max(n, 1)), np.uint16)
    _capi.check(lib.da_mh_counts(res.ctypes.data, off.ctypes.data, n, k, n_hash, seeds.ctypes.data,
                                 row_begin, row_end, out.ctypes.data))
    return out[:max(row_end - row_begin, 0), :n]


def similarityNW(sequences, matrixName="BLOSUM62", gapOpen=10, gapExt=4, *, devices=None, exchange=None):
    """Fraction identity (matches / alignment length) of the reference's
    affine-gap global alignment, all pairs.

    Mirrors reference ``similarityNW`` (src/pairwiseSeqAlign.cpp:331-365): no input
    validation beyond "Invalid substitution matrix name: %s" and the lazily raised
    "Invalid amino acid in sequence1/2: %c"; n == 0 gives a 0 x 0 matrix.
    devices= / exchange=: as for similarityMH (da_similarity_nw_opts)."""
    lib = _capi.load()
    res, off = pack_sequences(sequences)
    n = len(off) - 1
    out = np.empty((max(n, 1), max(n, 1)), np.float64)
    name = _matrix_name(matrixName)
    opts, keep = _device_opts(devices, exchange)
    if opts is None:
        _capi.check(lib.da_similarity_nw(res.ctypes.data, off.ctypes.data, n, name, _as_int(gapOpen, "gapOpen"),
                                         _as_int(gapExt, "gapExt"), out.ctypes.data))
    else:
        _capi.check(lib.da_similarity_nw_opts(res.ctypes.data, off.ctypes.data, n, name, _as_int(gapOpen, "gapOpen"),
                                              _as_int(gapExt, "gapExt"), out.ctypes.data, ctypes.addressof(opts)))
    _record_phases(keep)
    return SimilarityMatrix(out[:n, :n])


def similarityNW_cross(x, y, matrixName="BLOSUM62", gapOpen=10, gapExt=4):
    """Fraction identity of every sequence of ``x`` against every sequence of ``y``: the (m, n) matrix
    R[i, j] = calc(x[i], y[j]) with x[i] as sequence1 (the alignment is not symmetric) -- bit for bit the block
    [0:m, m:m+n] of ``similarityNW(x + y, ...)``.  An empty ``x`` or ``y`` gives a (0, n) / (m, 0) matrix; residue errors are
    what the reference's lazy fill would raise first with the pairs visited i over ``x``, then j over ``y``."""
    lib = _capi.load()
    xr, xo, m, yr, yo, n = _pack_two(x, y)
    out = np.empty((max(m, 1), max(n, 1)), np.float64)
    name = _matrix_name(matrixName)
    _capi.check(lib.da_similarity_nw_cross(xr.ctypes.data, xo.ctypes.data, m, yr.ctypes.data, yo.ctypes.data, n, name,
                                           _as_int(gapOpen, "gapOpen"), _as_int(gapExt, "gapExt"), out.ctypes.data, 0))
    return SimilarityMatrix(out[:m, :n])


def _nw_cross_topk(entry, x, y, matrixName, gapOpen, gapExt, top):
    lib = _capi.load()
    xr, xo, m, yr, yo, n = _pack_two(x, y)
    t, idx, val = _topk_arrays(m, top, n)
    name = _matrix_name(matrixName)
    _capi.check(getattr(lib, entry)(xr.ctypes.data, xo.ctypes.data, m, yr.ctypes.data, yo.ctypes.data, n, name,
                                    _as_int(gapOpen, "gapOpen"), _as_int(gapExt, "gapExt"), t, idx.ctypes.data, val.ctypes.data))
    return idx[:m, :max(t, 0)], val[:m, :max(t, 0)]


def similarityNW_cross_topk(x, y, matrixName="BLOSUM62", gapOpen=10, gapExt=4, top=10):
    """For every sequence of ``x`` its ``top`` most similar sequences of ``y`` under similarityNW_cross (x[i] is sequence1), without
    the (m, n) matrix: ``(idx, val)`` as similarityMH_cross_topk.  Equal similarities tie whatever their (matches, length): 2/4 and 3/6
    are both 0.5 and are listed by position.  Every sequence has 1 .. 127 residues (an empty one is refused: its similarities are NaN /
    0.0).  An empty ``x`` gives (0, top) arrays; ``top`` is clamped to ``len(y)``; an empty ``y`` is an error."""
    return _nw_cross_topk("da_similarity_nw_cross_topk", x, y, matrixName, gapOpen, gapExt, top)


def similarityNW_cross_topk_long(x, y, matrixName="BLOSUM62", gapOpen=10, gapExt=4, top=10):
    """``similarityNW_cross_topk`` for sequences of 1 .. 1024 residues (da_similarity_nw_cross_topk_long): the same arguments, the same
    result, the same errors.  The selection works on 32-bit value ranks (nw_value_ranks), so 128/256 and 150/300 tie and are listed by
    position; the (m, n) matrix never exists."""
    return _nw_cross_topk("da_similarity_nw_cross_topk_long", x, y, matrixName, gapOpen, gapExt, top)


def similarityMH_knn(sequences, k=4, n_hash=50, top=10, *, seed=None):
    """For every sequence its ``top`` most similar OTHER sequences under similarityMH, without the (n, n) matrix: ``(idx, val)``, (n, top)
    int32 0-based positions and the (n, top) float64 similarities, with ``(idx, val) == knn_dense(similarityMH(sequences, k, n_hash,
    seed=seed), top)``: value descending, position ascending among equals, the row's own position left out; columns of similarity 0 fill a
    row.  ``top`` is clamped to ``len(sequences) - 1`` (the C ABI does not clamp) and may be at most 1024.  Byte-identical sequences fill each
    other's lists at 1.0: pass distinct sequences.  Errors as similarityMH, then "a nearest neighbour needs a second sequence"."""
    lib, res, off, n, k, n_hash, seeds = _mh_prelude(sequences, k, n_hash, seed)
    t, idx, val = _topk_arrays(n, top, n - 1)
    _capi.check(lib.da_similarity_mh_knn(res.ctypes.data, off.ctypes.data, n, k, n_hash, seeds.ctypes.data, t, idx.ctypes.data, val.ctypes.data))
    return idx[:n], val[:n]


def _nw_knn(entry, sequences, matrixName, gapOpen, gapExt, top):
    lib = _capi.load()
    res, off = pack_sequences(sequences)
    n = len(off) - 1
    t, idx, val = _topk_arrays(n, top, n - 1)
    diag = np.empty(max(n, 1), np.float64)
    name = _matrix_name(matrixName)
    _capi.check(getattr(lib, entry)(res.ctypes.data, off.ctypes.data, n, name, _as_int(gapOpen, "gapOpen"), _as_int(gapExt, "gapExt"), t,
                                    idx.ctypes.data, val.ctypes.data, diag.ctypes.data))
    return idx[:n], val[:n], diag[:n]


def similarityNW_knn(sequences, matrixName="BLOSUM62", gapOpen=10, gapExt=4, top=10):
    """For every sequence its ``top`` most similar OTHER sequences under similarityNW, without the (n, n) matrix: ``(idx, val)`` as
    similarityMH_knn, ``== knn_dense(similarityNW(sequences, ...), top)``.  Equal similarities tie whatever their (matches, length).  Every
    sequence has 1 .. 127 residues (an empty one is refused); ``top`` is clamped to ``len(sequences) - 1``."""
    idx, val, _ = _nw_knn("da_similarity_nw_knn", sequences, matrixName, gapOpen, gapExt, top)
    return idx, val


def similarityNW_knn_long(sequences, matrixName="BLOSUM62", gapOpen=10, gapExt=4, top=10):
    """``similarityNW_knn`` for sequences of 1 .. 1024 residues (da_similarity_nw_knn_long): the same arguments, the same result
    ``== knn_dense(similarityNW(sequences, ...), top)``, the same errors.  The selection works on 32-bit value ranks (nw_value_ranks); the
    (n, n) matrix never exists.  A set that does not fit one block of DYNAALIGN_BLOCK_BYTES computes every pair twice."""
    idx, val, _ = _nw_knn("da_similarity_nw_knn_long", sequences, matrixName, gapOpen, gapExt, top)
    return idx, val


def knn_dense(S, top):
    """The nearest-neighbour lists of a dense symmetric similarity matrix, the definition in numpy: ``(idx, val)`` with
    ``idx = argsort(-S', axis=1, kind="stable")[:, :top]`` for S' = S with its diagonal at -inf (int32) and ``val[i, t] = S[i, idx[i, t]]``.
    1 <= top <= n - 1.  The counterpart of similarityMH_knn / similarityNW_knn, as compute_similarity_stats is of the *_stats calls."""
    S = np.asarray(S, np.float64)
    if S.ndim != 2 or S.shape[0] != S.shape[1]:
        raise ValueError("Input must be a square pairwise similarity matrix")
    n = S.shape[0]
    top = _as_int(top, "top")
    if n < 2:
        raise ValueError("a nearest neighbour needs a second sequence")
    if not 1 <= top <= n - 1:
        raise ValueError("top must be in 1 .. n - 1 (got top = %d, n = %d)" % (top, n))
    M = np.array(S, np.float64)
    np.fill_diagonal(M, -np.inf)
    idx = np.argsort(-M, axis=1, kind="stable")[:, :top]
    return idx.astype(np.int32), np.take_along_axis(np.asarray(S, np.float64), idx, axis=1)


def knn_graph(idx, val, diag=None, mode="union"):
    """Nearest-neighbour lists -> the edge list ``(i, j, w)`` of their kNN graph, i <= j, sorted by (i, j), pure numpy.  An entry (i -> j) is live
    when ``val > 0``; ``mode="union"`` keeps the pair {i, j} when j is live in row i or i is live in row j, ``"mutual"`` when both hold; the
    weight is the listed value.  ``diag`` (n values, or a scalar) adds the entries (i, i, diag[i]); ``diag=None`` adds none.  This is the
    adjacency netcluster builds from the similarity matrix with every off-diagonal entry outside the kNN relation set to 0, in the form
    ``clusterbreak(edges_fn=)`` takes."""
    if mode not in ("union", "mutual"):
        raise ValueError("mode must be 'union' or 'mutual'")
    idx = np.asarray(idx, np.int64)
    val = np.asarray(val, np.float64)
    if idx.ndim != 2 or idx.shape != val.shape:
        raise ValueError("idx and val must be (n, top) arrays of one shape")
    n = idx.shape[0]
    rows = np.repeat(np.arange(n, dtype=np.int64), idx.shape[1])
    cols, w = idx.ravel(), val.ravel()
    live = (w > 0) & (cols != rows)
    rows, cols, w = rows[live], cols[live], w[live]
    lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
    pair = lo * n + hi
    order = np.argsort(pair, kind="stable")
    pair, w = pair[order], w[order]
    first = np.ones(len(pair), bool)
    first[1:] = pair[1:] != pair[:-1]
    if mode == "mutual":                       # a pair listed from both sides appears twice
        twice = np.zeros(len(pair), bool)
        twice[:-1] = pair[1:] == pair[:-1]
        first &= twice
    pair, w = pair[first], w[first]
    ei, ej = pair // max(n, 1), pair % max(n, 1)
    if diag is not None:
        d = np.broadcast_to(np.asarray(diag, np.float64), (n,))
        ei = np.concatenate([ei, np.arange(n, dtype=np.int64)])
        ej = np.concatenate([ej, np.arange(n, dtype=np.int64)])
        w = np.concatenate([w, d])
        order = np.lexsort((ej, ei))
        ei, ej, w = ei[order], ej[order], w[order]
    return ei.astype(np.int32), ej.astype(np.int32), np.ascontiguousarray(w, np.float64)


def _knn_edges_result(idx, val, diag, mode):
    ei, ej, w = knn_graph(idx, val, diag, mode)
    off = w[ei != ej]
    return (float(off.min()) if len(off) else float("nan")), ei, ej, w


def similarityMH_knn_edges(sequences, k=4, n_hash=50, top=10, mode="union", *, seed=None):
    """The kNN graph of similarityMH_knn as ``(threshold, i, j, w)`` for ``clusterbreak(edges_fn=)``: knn_graph of the lists with the 1.0
    diagonal of similarityMH.  The ``threshold`` slot holds the smallest off-diagonal weight kept, NaN when none."""
    idx, val = similarityMH_knn(sequences, k, n_hash, top, seed=seed)
    return _knn_edges_result(idx, val, 1.0, mode)


def similarityNW_knn_edges(sequences, matrixName="BLOSUM62", gapOpen=10, gapExt=4, top=10, mode="union"):
    """The kNN graph of similarityNW_knn as ``(threshold, i, j, w)`` for ``clusterbreak(edges_fn=)``; the diagonal is what the DP gives for a
    sequence against itself.  The ``threshold`` slot holds the smallest off-diagonal weight kept, NaN when none."""
    idx, val, diag = _nw_knn("da_similarity_nw_knn", sequences, matrixName, gapOpen, gapExt, top)
    return _knn_edges_result(idx, val, diag, mode)


def similarityNW_knn_edges_long(sequences, matrixName="BLOSUM62", gapOpen=10, gapExt=4, top=10, mode="union"):
    """``similarityNW_knn_edges`` for sequences of 1 .. 1024 residues: the kNN graph of similarityNW_knn_long with the DP's diagonal.
    ``clusterbreak(pep, edges_fn=lambda s: similarityNW_knn_edges_long(s, top=10))`` clusters full-length proteins on it."""
    idx, val, diag = _nw_knn("da_similarity_nw_knn_long", sequences, matrixName, gapOpen, gapExt, top)
    return _knn_edges_result(idx, val, diag, mode)


def _byte_strings(sequences):
    if isinstance(sequences, (str, bytes)):
        sequences = [sequences]
    return [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in sequences]


def jaccard_counts(sequences, k, y=None):
    """``(intersection, union)``, two int64 matrices: the sizes of S_k(a) & S_k(b) and S_k(a) | S_k(b) for every sequence a of ``sequences``
    against every b of ``y`` (``y=None``: of ``sequences``), S_k(s) the set of distinct length-k byte substrings of s (empty when
    len(s) < k).  Plain Python sets, for small inputs: the integers behind jaccard_dense and behind the device's uint16 code
    ``intersection << 8 | union`` (two empty sets are coded 0x0101)."""
    k = _as_int(k, "k")
    if k < 1:
        raise ValueError("'k' must be a positive integer")
    xs = [{b[p:p + k] for p in range(len(b) - k + 1)} for b in _byte_strings(sequences)]
    ys = xs if y is None else [{b[p:p + k] for p in range(len(b) - k + 1)} for b in _byte_strings(y)]
    inter = np.zeros((len(xs), len(ys)), np.int64)
    union = np.zeros((len(xs), len(ys)), np.int64)
    for i, a in enumerate(xs):
        for j, b in enumerate(ys):
            c = len(a & b)
            inter[i, j] = c
            union[i, j] = len(a) + len(b) - c
    return inter, union


def jaccard_dense(sequences, k, y=None):
    """The exact Jaccard index of k-shingle sets, the definition in Python: the float64 matrix J[i, j] = intersection / union of
    jaccard_counts -- one IEEE divide of the two integers -- 1.0 where both sets are empty, 0.0 where exactly one is.  The counterpart of
    similarityJaccard / similarityJaccard_cross, as knn_dense is of the *_knn calls; no limit on k or the lengths, small inputs only."""
    inter, union = jaccard_counts(sequences, k, y)
    out = np.ones(inter.shape, np.float64)
    np.divide(inter.astype(np.float64), union.astype(np.float64), out=out, where=union > 0)
    return out


def similarityJaccard(sequences, k=4):
    """The exact Jaccard index of the k-shingle sets of all pairs: what similarityMH estimates with ``n_hash`` hash functions, computed without
    them -- no seed, no estimator noise, diagonal 1.0 by the definition.  ``== jaccard_dense(sequences, k)`` bit for bit.  k <= 8 and every
    sequence has at most 127 shingle positions (``len - k + 1 <= 127``); empty sequences and sequences shorter than k are legal (two empty
    sets give 1.0, one gives 0.0).  Errors "Input sequences vector cannot be empty", "'k' must be a positive integer" as similarityMH."""
    return _jaccard_square("da_similarity_jaccard", sequences, k)


def _jaccard_square(entry, sequences, k):
    lib = _capi.load()
    res, off = pack_sequences(sequences)
    n = len(off) - 1
    out = np.empty((max(n, 1), max(n, 1)), np.float64)
    _capi.check(getattr(lib, entry)(res.ctypes.data, off.ctypes.data, n, _as_int(k, "k"), out.ctypes.data))
    return SimilarityMatrix(out[:n, :n])


def similarityJaccard_cross(x, y, k=4):
    """The exact Jaccard index of every sequence of ``x`` against every sequence of ``y``: the (m, n) matrix, bit for bit the block
    [0:m, m:m+n] of ``similarityJaccard(x + y, k)``.  An empty ``x`` or ``y`` gives a (0, n) / (m, 0) matrix."""
    return _jaccard_cross("da_similarity_jaccard_cross", x, y, k)


def _jaccard_cross(entry, x, y, k):
    lib = _capi.load()
    xr, xo, m, yr, yo, n = _pack_two(x, y)
    out = np.empty((max(m, 1), max(n, 1)), np.float64)
    _capi.check(getattr(lib, entry)(xr.ctypes.data, xo.ctypes.data, m, yr.ctypes.data, yo.ctypes.data, n, _as_int(k, "k"), out.ctypes.data, 0))
    return SimilarityMatrix(out[:m, :n])


def similarityJaccard_cross_topk(x, y, k=4, top=10):
    """For every sequence of ``x`` its ``top`` most similar sequences of ``y`` under similarityJaccard_cross, without the (m, n) matrix:
    ``(idx, val)`` as similarityMH_cross_topk, ``idx == np.argsort(-R, axis=1, kind="stable")[:, :top]``.  Equal values tie whatever their
    (intersection, union): 2/4 and 3/6 are listed by position.  An empty ``x`` gives (0, top) arrays; ``top`` is clamped to ``len(y)``; an
    empty ``y`` is an error."""
    return _jaccard_cross_topk("da_similarity_jaccard_cross_topk", x, y, k, top)


def _jaccard_cross_topk(entry, x, y, k, top):
    lib = _capi.load()
    xr, xo, m, yr, yo, n = _pack_two(x, y)
    t, idx, val = _topk_arrays(m, top, n)
    _capi.check(getattr(lib, entry)(xr.ctypes.data, xo.ctypes.data, m, yr.ctypes.data, yo.ctypes.data, n, _as_int(k, "k"), t, idx.ctypes.data,
                                    val.ctypes.data))
    return idx[:m, :max(t, 0)], val[:m, :max(t, 0)]


def similarityJaccard_knn(sequences, k=4, top=10):
    """For every sequence its ``top`` most similar OTHER sequences under similarityJaccard, without the (n, n) matrix: ``(idx, val) ==
    knn_dense(similarityJaccard(sequences, k), top)``.  ``top`` is clamped to ``len(sequences) - 1`` and may be at most 1024.  Sequences with
    equal shingle sets fill each other's lists at 1.0."""
    return _jaccard_knn("da_similarity_jaccard_knn", sequences, k, top)


def _jaccard_knn(entry, sequences, k, top):
    lib = _capi.load()
    res, off = pack_sequences(sequences)
    n = len(off) - 1
    t, idx, val = _topk_arrays(n, top, n - 1)
    _capi.check(getattr(lib, entry)(res.ctypes.data, off.ctypes.data, n, _as_int(k, "k"), t, idx.ctypes.data, val.ctypes.data))
    return idx[:n], val[:n]


def similarityJaccard_knn_edges(sequences, k=4, top=10, mode="union"):
    """The kNN graph of similarityJaccard_knn as ``(threshold, i, j, w)`` for ``clusterbreak(edges_fn=)``: knn_graph of the lists with the 1.0
    diagonal the definition gives.  The ``threshold`` slot holds the smallest off-diagonal weight kept, NaN when none."""
    idx, val = similarityJaccard_knn(sequences, k, top)
    return _knn_edges_result(idx, val, 1.0, mode)


def similarityJaccard_edges(sequences, k=4, thresh_p=0.8):
    """similarityJaccard followed by clusterbreak's threshold step (reference R/clusterbreak.R:217-221), fused on the device like
    similarityMH_edges: ``(threshold, i, j, weight)`` for the entries with i <= j (0-based, sorted, diagonal included) whose value is
    >= the type-7 ``thresh_p`` quantile of the strict upper triangle and > 0.  A deterministic graph for
    ``clusterbreak(pep, edges_fn=lambda s: similarityJaccard_edges(s, k=2))``."""
    return _jaccard_edges("da_similarity_jaccard_edges_begin", sequences, k, thresh_p)


def _jaccard_edges(entry, sequences, k, thresh_p):
    lib = _capi.load()
    res, off = pack_sequences(sequences)
    n = len(off) - 1
    k = _as_int(k, "k")
    return _edges_one_pass(lambda h, thr, cnt: getattr(lib, entry)(res.ctypes.data, off.ctypes.data, n, k, float(thresh_p), h, thr, cnt))


# ---- the exact Jaccard index for sequences of up to 1024 shingle positions: the _long siblings ------------------------------------------------

def similarityJaccard_long(sequences, k=4):
    """``similarityJaccard`` for sequences of up to 1024 shingle positions, ``len - k + 1 <= 1024`` (da_similarity_jaccard_long): the same
    arguments, the same result bit for bit -- ``== jaccard_dense(sequences, k)`` -- the same errors with 1024 in place of 127.  What an
    ``n_hash = 50`` similarityMH estimate of full-length proteins is measured against."""
    return _jaccard_square("da_similarity_jaccard_long", sequences, k)


def similarityJaccard_cross_long(x, y, k=4):
    """``similarityJaccard_cross`` for sequences of up to 1024 shingle positions (da_similarity_jaccard_cross_long)."""
    return _jaccard_cross("da_similarity_jaccard_cross_long", x, y, k)


def similarityJaccard_cross_topk_long(x, y, k=4, top=10):
    """``similarityJaccard_cross_topk`` for sequences of up to 1024 shingle positions (da_similarity_jaccard_cross_topk_long): the selection
    runs on 32-bit value ranks (``nw_value_ranks`` of the call's largest shingle count) of the codes ``intersection << 16 | union``."""
    return _jaccard_cross_topk("da_similarity_jaccard_cross_topk_long", x, y, k, top)


def similarityJaccard_knn_long(sequences, k=4, top=10):
    """``similarityJaccard_knn`` for sequences of up to 1024 shingle positions (da_similarity_jaccard_knn_long): ``(idx, val) ==
    knn_dense(similarityJaccard_long(sequences, k), top)`` without the (n, n) matrix."""
    return _jaccard_knn("da_similarity_jaccard_knn_long", sequences, k, top)


def similarityJaccard_knn_edges_long(sequences, k=4, top=10, mode="union"):
    """``similarityJaccard_knn_edges`` for sequences of up to 1024 shingle positions: knn_graph of similarityJaccard_knn_long's lists with
    the 1.0 diagonal, as ``(threshold, i, j, w)`` for ``clusterbreak(edges_fn=)``."""
    idx, val = similarityJaccard_knn_long(sequences, k, top)
    return _knn_edges_result(idx, val, 1.0, mode)


def similarityJaccard_edges_long(sequences, k=4, thresh_p=0.8):
    """``similarityJaccard_edges`` for sequences of up to 1024 shingle positions (da_similarity_jaccard_edges_long_begin): the same
    arguments, the same result, the same errors.  ``clusterbreak(pep, edges_fn=lambda s: similarityJaccard_edges_long(s, k=4))`` clusters
    full-length proteins on the exact index."""
    return _jaccard_edges("da_similarity_jaccard_edges_long_begin", sequences, k, thresh_p)


def similarityJaccard_cross_edges_long(x, y, k=4, thresh_p=0.8, *, threshold=None):
    """The entries of R = similarityJaccard_cross_long(x, y, k) that pass a threshold, without the (m, n) matrix: ``(threshold, i, j,
    weight)`` as similarityMH_cross_edges -- every (i, j) with ``R[i, j] >= threshold and R[i, j] > 0``, sorted by (i, j), ``weight`` bit
    for bit ``R[i, j]``; ``threshold=None`` takes R's type-7 ``thresh_p`` quantile over all m * n entries.  Sequences of up to 1024
    shingle positions, short ones included (the short family has no such form).  An empty ``x`` or ``y`` gives no edges in the absolute
    form and is an error in the quantile form."""
    lib = _capi.load()
    xr, xo, m, yr, yo, n = _pack_two(x, y)
    k = _as_int(k, "k")
    thresh, is_q = _thresh_args(thresh_p, threshold)
    return _edges_one_pass(lambda h, thr, cnt: lib.da_similarity_jaccard_cross_edges_long_begin(
        xr.ctypes.data, xo.ctypes.data, m, yr.ctypes.data, yo.ctypes.data, n, k, thresh, is_q, h, thr, cnt))


def similarityJaccard_stats_long(sequences, k=4):
    """``compute_similarity_stats(similarityJaccard_long(sequences, k))`` without the matrix on the host (da_similarity_jaccard_stats_long):
    one pass of the rectangle kernel in row blocks, on 32-bit value ranks.  Empty sequences are legal (two empty sets are 1.0)."""
    lib = _capi.load()
    res, off = pack_sequences(sequences)
    n = len(off) - 1
    s = _capi.DaSimilarityStats()
    _capi.check(lib.da_similarity_jaccard_stats_long(res.ctypes.data, off.ctypes.data, n, _as_int(k, "k"), ctypes.addressof(s)))
    return _stats_result(s)


# ---- the Levenshtein similarity: plain edit distance ------------------------------------------------------------------------------------------

def lev_counts(sequences, y=None):
    """``(L - d, L)``, two int64 matrices, for every sequence a of ``sequences`` against every b of ``y`` (``y=None``: of ``sequences``):
    d the Levenshtein distance of the two byte strings -- insert, delete and substitute cost 1 each -- and L the longer of the two lengths.
    The plain O(len(a) len(b)) dynamic programme, for small inputs: the integers behind lev_dense and behind the device's uint16 code
    ``(L - d) << 8 | L`` (two empty strings are coded 0x0101)."""
    xs = _byte_strings(sequences)
    ys = xs if y is None else _byte_strings(y)
    num = np.zeros((len(xs), len(ys)), np.int64)
    den = np.zeros((len(xs), len(ys)), np.int64)
    for i, a in enumerate(xs):
        ta = np.frombuffer(a, np.uint8)
        for j, b in enumerate(ys):
            prev = np.arange(len(a) + 1, dtype=np.int64)             # d(a[:p], "") = p
            for q in range(len(b)):
                # substitute or match, delete from b; then the inserts along the column as a running minimum
                cur = np.empty_like(prev)
                cur[0] = q + 1
                np.minimum(prev[:-1] + (ta != b[q]), prev[1:] + 1, out=cur[1:])
                cur = np.minimum.accumulate(cur - np.arange(len(cur))) + np.arange(len(cur))
                prev = cur
            longer = max(len(a), len(b))
            num[i, j] = longer - int(prev[-1])
            den[i, j] = longer
    return num, den


def lev_dense(sequences, y=None):
    """The Levenshtein similarity, the definition in Python: the float64 matrix ``(L - d) / L`` of lev_counts -- one IEEE divide of the two
    integers -- 1.0 for two empty strings, 0.0 where exactly one is empty.  The counterpart of similarityLev / similarityLev_cross, as
    jaccard_dense is of similarityJaccard; no limit on the lengths, small inputs only."""
    num, den = lev_counts(sequences, y)
    out = np.ones(num.shape, np.float64)
    np.divide(num.astype(np.float64), den.astype(np.float64), out=out, where=den > 0)
    return out


def similarityLev(sequences):
    """The Levenshtein similarity of all pairs: ``(L - d) / L`` with d the unit-cost edit distance of the two byte strings and L the longer
    length; ``== lev_dense(sequences)`` bit for bit, diagonal 1.0 by the definition, symmetric.  Any byte values (``str`` goes through
    latin-1), every sequence at most 127 bytes; the empty string is legal (two of them give 1.0, one gives 0.0).  With all strings of
    length L, the pairs within t edits are those at or above ``(L - t) / L``."""
    lib = _capi.load()
    res, off = pack_sequences(sequences)
    n = len(off) - 1
    out = np.empty((max(n, 1), max(n, 1)), np.float64)
    _capi.check(lib.da_similarity_lev(res.ctypes.data, off.ctypes.data, n, out.ctypes.data))
    return SimilarityMatrix(out[:n, :n])


def similarityLev_cross(x, y):
    """The Levenshtein similarity of every sequence of ``x`` against every sequence of ``y``: the (m, n) matrix, bit for bit the block
    [0:m, m:m+n] of ``similarityLev(x + y)``.  An empty ``x`` or ``y`` gives a (0, n) / (m, 0) matrix."""
    lib = _capi.load()
    xr, xo, m, yr, yo, n = _pack_two(x, y)
    out = np.empty((max(m, 1), max(n, 1)), np.float64)
    _capi.check(lib.da_similarity_lev_cross(xr.ctypes.data, xo.ctypes.data, m, yr.ctypes.data, yo.ctypes.data, n, out.ctypes.data, 0))
    return SimilarityMatrix(out[:m, :n])


def similarityLev_cross_topk(x, y, top=10):
    """For every sequence of ``x`` its ``top`` most similar sequences of ``y`` under similarityLev_cross, without the (m, n) matrix:
    ``(idx, val)`` as similarityJaccard_cross_topk, ``idx == np.argsort(-R, axis=1, kind="stable")[:, :top]``.  Equal values tie whatever
    their (L - d, L): 10/20 and 5/10 are listed by position.  An empty ``x`` gives (0, top) arrays; ``top`` is clamped to ``len(y)``; an
    empty ``y`` is an error."""
    lib = _capi.load()
    xr, xo, m, yr, yo, n = _pack_two(x, y)
    t, idx, val = _topk_arrays(m, top, n)
    _capi.check(lib.da_similarity_lev_cross_topk(xr.ctypes.data, xo.ctypes.data, m, yr.ctypes.data, yo.ctypes.data, n, t, idx.ctypes.data,
                                                 val.ctypes.data))
    return idx[:m, :max(t, 0)], val[:m, :max(t, 0)]


def similarityLev_knn(sequences, top=10):
    """For every sequence its ``top`` most similar OTHER sequences under similarityLev, without the (n, n) matrix: ``(idx, val) ==
    knn_dense(similarityLev(sequences), top)``.  ``top`` is clamped to ``len(sequences) - 1`` and may be at most 1024.  Byte-identical
    strings fill each other's lists at 1.0."""
    lib = _capi.load()
    res, off = pack_sequences(sequences)
    n = len(off) - 1
    t, idx, val = _topk_arrays(n, top, n - 1)
    _capi.check(lib.da_similarity_lev_knn(res.ctypes.data, off.ctypes.data, n, t, idx.ctypes.data, val.ctypes.data))
    return idx[:n], val[:n]


def similarityLev_knn_edges(sequences, top=10, mode="union"):
    """The kNN graph of similarityLev_knn as ``(threshold, i, j, w)`` for ``clusterbreak(edges_fn=)``: knn_graph of the lists with the 1.0
    diagonal the definition gives.  The ``threshold`` slot holds the smallest off-diagonal weight kept, NaN when none."""
    idx, val = similarityLev_knn(sequences, top)
    return _knn_edges_result(idx, val, 1.0, mode)


def similarityLev_edges(sequences, thresh_p=0.8):
    """similarityLev followed by clusterbreak's threshold step (reference R/clusterbreak.R:217-221), fused on the device like
    similarityJaccard_edges: ``(threshold, i, j, weight)`` for the entries with i <= j (0-based, sorted, diagonal included) whose value is
    >= the type-7 ``thresh_p`` quantile of the strict upper triangle and > 0.  An order-aware graph at bit-vector cost for
    ``clusterbreak(pep, edges_fn=lambda s: similarityLev_edges(s))``."""
    lib = _capi.load()
    res, off = pack_sequences(sequences)
    n = len(off) - 1
    return _edges_one_pass(lambda h, thr, cnt: lib.da_similarity_lev_edges_begin(res.ctypes.data, off.ctypes.data, n, float(thresh_p), h, thr, cnt))


def similarityLev_cross_edges(x, y, thresh_p=0.8, *, threshold=None):
    """The range query: the entries of R = similarityLev_cross(x, y) that pass a threshold, without the (m, n) matrix: ``(threshold, i, j,
    weight)`` as similarityNW_cross_edges -- every (i, j) with ``R[i, j] >= threshold and R[i, j] > 0``, sorted by (i, j), ``weight`` bit
    for bit ``R[i, j]``; ``threshold=None`` takes R's type-7 ``thresh_p`` quantile over all m * n entries.  With all strings of length L,
    ``threshold=(L - t) / L`` lists every pair within t edits.  An empty ``x`` or ``y`` gives no edges in the absolute form and is an
    error in the quantile form."""
    lib = _capi.load()
    xr, xo, m, yr, yo, n = _pack_two(x, y)
    thresh, is_q = _thresh_args(thresh_p, threshold)
    return _edges_one_pass(lambda h, thr, cnt: lib.da_similarity_lev_cross_edges_begin(
        xr.ctypes.data, xo.ctypes.data, m, yr.ctypes.data, yo.ctypes.data, n, thresh, is_q, h, thr, cnt))


def nw_code_ranks(max_len=127):
    """(ranks uint16[65536], distinct): the dense value rank of every NW code (matches << 8 | length) sequences up to max_len residues
    can produce -- what similarityNW_cross_topk selects on (da_nw_code_ranks).  Needs no device."""
    out = np.zeros(65536, np.uint16)
    d = ctypes.c_int(0)
    _capi.check(_capi.load().da_nw_code_ranks(int(max_len), out.ctypes.data, ctypes.addressof(d)))
    return out, d.value


def nw_value_ranks(max_len=1024):
    """(values float64[D], rank uint32[2 * max_len + 1, max_len + 1]): the distinct values ``matches / length`` that sequences of up to max_len
    (1 .. 1024) residues can produce, ascending, and ``rank[length, matches]``, the dense rank of that value -- what the *_edges_long calls
    order and threshold on (da_nw_value_ranks).  Equal doubles share a rank (128/256 and 150/300); rank 0 is the value 0.0.  Needs no device."""
    lib = _capi.load()
    ml = int(max_len)
    d = ctypes.c_int64(0)
    _capi.check(lib.da_nw_value_ranks(ml, None, ctypes.addressof(d), None))
    values = np.empty(d.value, np.float64)
    rank = np.empty((2 * ml + 1, ml + 1), np.uint32)
    _capi.check(lib.da_nw_value_ranks(ml, values.ctypes.data, ctypes.addressof(d), rank.ctypes.data))
    return values, rank


def nw_pairs(sequences, matrixName="BLOSUM62", gapOpen=10, gapExt=4, *, row_begin=0, row_end=None):
    """(matches, length, score) int32 arrays for a row block: the integers the
    reference divides at src/pairwiseSeqAlign.cpp:311, plus M[m][n]."""
    lib = _capi.load()
    res, off = pack_sequences(sequences)
    n = len(off) - 1
    row_end = n if row_end is None else row_end
    r = max(row_end - row_begin, 0)
    mt = np.zeros((max(r, 1), max(n, 1)), np.int32)
    ln = np.zeros_like(mt)
    sc = np.zeros_like(mt)
    name = _matrix_name(matrixName)
    _capi.check(lib.da_nw_pairs(res.ctypes.data, off.ctypes.data, n, name, _as_int(gapOpen, "gapOpen"),
                                _as_int(gapExt, "gapExt"), row_begin, row_end, mt.ctypes.data, ln.ctypes.data,
                                sc.ctypes.data))
    return mt[:r, :n], ln[:r, :n], sc[:r, :n]


class NWAlignment(tuple):
    """Result of nw_align: a tuple ``(ops, length, matches, score)`` with the same fields as attributes."""
    __slots__ = ()

    def __new__(cls, ops, length, matches, score):
        return tuple.__new__(cls, (ops, length, matches, score))

    ops = property(lambda self: self[0])
    length = property(lambda self: self[1])
    matches = property(lambda self: self[2])
    score = property(lambda self: self[3])


def nw_align(x, y, matrixName="BLOSUM62", gapOpen=10, gapExt=4, *, pairs=None, ops=True):
    """HOW listed pairs align under the reference's affine-gap global alignment (da_nw_align_pairs): pair p aligns ``x[i_idx[p]]`` as
    sequence1 with ``y[j_idx[p]]`` as sequence2, ``pairs=(i_idx, j_idx)`` (0-based, repeats allowed); without ``pairs`` pair p is
    ``x[p]`` with ``y[p]`` and ``len(x) == len(y)`` is required (ValueError otherwise).  Returns ``(ops, length, matches, score)``
    (also as attributes):

        ops      list of str over "DUL", the path from the start of both sequences to their ends -- D: x's residue opposite y's,
                 U: x's residue opposite a gap, L: a gap opposite y's residue (``nw_align_strings`` renders it) -- or None with ops=False
        length   int32, len(ops[p]): the reference's alignment_length        matches  int32, D steps with equal residues
        score    int32, M[m][n] after the fill

    ``matches / length`` is bit for bit ``similarityNW_cross(x, y)[i, j]``.  The path is the one the reference's traceback walks
    (src/pairwiseSeqAlign.cpp:271-308), ties included.  Sequences have 0 .. 127 residues; errors as similarityNW_cross, raised for the
    listed sequences only."""
    return _nw_align_call("da_nw_align_pairs", 254, x, y, matrixName, gapOpen, gapExt, pairs, ops)


def nw_align_long(x, y, matrixName="BLOSUM62", gapOpen=10, gapExt=4, *, pairs=None, ops=True):
    """``nw_align`` for sequences of 0 .. 1024 residues (da_nw_align_long_pairs): the same arguments, the same result, the same errors.
    Listed pairs with both sequences of at most 127 residues run through ``nw_align``'s kernels, every other pair takes one wavefront
    (``k_nw_align_long``); the results come back in listed order.  The ops rows are as long as the longest listed ``len(x) + len(y)``.
    ``clusterconsensus(rows, align_fn=nw_align_long)`` builds consensus sequences with it."""
    return _nw_align_call("da_nw_align_long_pairs", None, x, y, matrixName, gapOpen, gapExt, pairs, ops)


def _nw_align_call(entry, ld_cap, x, y, matrixName, gapOpen, gapExt, pairs, ops):
    """nw_align / nw_align_long: marshal, call ``entry``, cut the ops rows into strings.  ld_cap: upper bound of the ops row length."""
    lib = _capi.load()
    xr, xo, m, yr, yo, n = _pack_two(x, y)
    if pairs is None:
        if m != n:
            raise ValueError("without pairs, x and y must have the same length (got %d and %d)" % (m, n))
        px = py = None
        count = m
        lens = np.diff(xo) + np.diff(yo)
    else:
        i_idx, j_idx = pairs
        px = np.clip(np.asarray(i_idx, np.int64).ravel(), -1, 2 ** 31 - 1).astype(np.int32)
        py = np.clip(np.asarray(j_idx, np.int64).ravel(), -1, 2 ** 31 - 1).astype(np.int32)
        if len(px) != len(py):
            raise ValueError("pairs must be two index lists of the same length (got %d and %d)" % (len(px), len(py)))
        count = len(px)
        # only to size the ops rows: the library checks the indices themselves
        lens = (np.diff(xo)[np.clip(px, 0, m - 1)] + np.diff(yo)[np.clip(py, 0, n - 1)]) if m > 0 and n > 0 else np.zeros(0, np.int64)
    ld = max(int(lens.max()) if len(lens) else 0, 1)
    if ld_cap is not None:
        ld = min(ld, ld_cap)
    buf = np.zeros((max(count, 1), ld), np.uint8) if ops else None
    ln = np.zeros(max(count, 1), np.int32)
    mt = np.zeros_like(ln)
    sc = np.zeros_like(ln)
    name = _matrix_name(matrixName)
    _capi.check(getattr(lib, entry)(xr.ctypes.data, xo.ctypes.data, m, yr.ctypes.data, yo.ctypes.data, n, _capi.ptr(px), _capi.ptr(py), count,
                                    name, _as_int(gapOpen, "gapOpen"), _as_int(gapExt, "gapExt"), _capi.ptr(buf), ld, ln.ctypes.data,
                                    mt.ctypes.data, sc.ctypes.data))
    ln, mt, sc = ln[:count], mt[:count], sc[:count]
    strings = None
    if ops:
        raw = buf.tobytes()
        strings = [raw[p * ld:p * ld + int(ln[p])].decode("latin-1") for p in range(count)]
    return NWAlignment(strings, ln, mt, sc)


def nw_align_strings(a, b, ops):
    """The two gapped strings of one alignment path (``nw_align``'s ops for sequence1 ``a`` and sequence2 ``b``): '-' opposite a U
    (in the second string) or an L (in the first), both of length len(ops).  Host only."""
    ga, gb = [], []
    i = j = 0
    for op in ops:
        if op == "D":
            ga.append(a[i]); gb.append(b[j]); i += 1; j += 1
        elif op == "U":
            ga.append(a[i]); gb.append("-"); i += 1
        elif op == "L":
            ga.append("-"); gb.append(b[j]); j += 1
        else:
            raise ValueError("ops holds %r: expected only 'D', 'U', 'L'" % op)
    if i != len(a) or j != len(b):
        raise ValueError("ops consumes %d and %d residues, the sequences have %d and %d" % (i, j, len(a), len(b)))
    return "".join(ga), "".join(gb)


def quantile_type7(hist, values, p):
    """R's quantile(x, p, type = 7) of {values[b] repeated hist[b] times} (values ascending)."""
    lib = _capi.load()
    h = np.ascontiguousarray(hist, np.uint64)
    v = np.ascontiguousarray(values, np.float64)
    q = np.zeros(1, np.float64)
    _capi.check(lib.da_quantile_type7(h.ctypes.data, v.ctypes.data, len(h), float(p), q.ctypes.data))
    return float(q[0])


def similarityMH_edges(sequences, k=4, n_hash=50, thresh_p=0.8, *, seed=None):
    """similarityMH followed by clusterbreak's threshold step, fused on the device.

    Equivalent to (reference R/clusterbreak.R:217-221, netcluster :122-124)

        S <- similarityMH(sequences, k, n_hash)
        threshold <- quantile(S[upper.tri(S)], thresh_p)
        S[S < threshold] <- 0                      # edges = non-zero entries of the upper triangle + diagonal

    but returns only ``(threshold, i, j, weight)`` -- the surviving entries with i <= j (0-based, sorted),
    never the dense matrix."""
    lib, res, off, n, k, n_hash, seeds = _mh_prelude(sequences, k, n_hash, seed)
    return _edges_one_pass(lambda h, thr, cnt: lib.da_similarity_mh_edges_begin(
        res.ctypes.data, off.ctypes.data, n, k, n_hash, seeds.ctypes.data, float(thresh_p), h, thr, cnt))


def _edges_one_pass(begin):
    """*_edges_begin -> da_edges_fetch -> da_edges_free: the pipeline runs once (the size-query form runs it twice)"""
    lib = _capi.load()
    handle = ctypes.c_void_p()
    thr = np.zeros(1, np.float64)
    cnt = np.zeros(1, np.int64)
    _capi.check(begin(ctypes.addressof(handle), thr.ctypes.data, cnt.ctypes.data))
    try:
        m = int(cnt[0])
        ei, ej, ew = np.empty(max(m, 1), np.int32), np.empty(max(m, 1), np.int32), np.empty(max(m, 1), np.float64)
        _capi.check(lib.da_edges_fetch(handle, m, ei.ctypes.data, ej.ctypes.data, ew.ctypes.data))
    finally:
        lib.da_edges_free(handle)
    return float(thr[0]), ei[:m], ej[:m], ew[:m]


def similarityNW_edges(sequences, matrixName="BLOSUM62", gapOpen=10, gapExt=4, thresh_p=0.8):
    """similarityNW followed by clusterbreak's threshold step (reference R/clusterbreak.R:217-221), fused on
    the device like similarityMH_edges: returns ``(threshold, i, j, weight)`` for the surviving entries with
    i <= j (0-based, sorted).  Sequences up to 127 residues; empty sequences are refused (NaN similarities)."""
    return _nw_edges("da_similarity_nw_edges_begin", sequences, matrixName, gapOpen, gapExt, thresh_p)


def _nw_edges(entry, sequences, matrixName, gapOpen, gapExt, thresh_p):
    lib = _capi.load()
    res, off = pack_sequences(sequences)
    n = len(off) - 1
    name = _matrix_name(matrixName)
    go, ge = _as_int(gapOpen, "gapOpen"), _as_int(gapExt, "gapExt")
    return _edges_one_pass(lambda h, thr, cnt: getattr(lib, entry)(res.ctypes.data, off.ctypes.data, n, name, go, ge, float(thresh_p), h, thr, cnt))


def similarityNW_edges_long(sequences, matrixName="BLOSUM62", gapOpen=10, gapExt=4, thresh_p=0.8):
    """``similarityNW_edges`` for sequences of 1 .. 1024 residues (da_similarity_nw_edges_long_begin): the same arguments, the same result,
    the same errors.  The device thresholds 32-bit value ranks (``nw_value_ranks``) of the packed (matches, length) pairs; the dense matrix
    never exists.  ``clusterbreak(pep, edges_fn=lambda s: similarityNW_edges_long(s, thresh_p=0.8), thresh_p=0.8)`` clusters with it."""
    return _nw_edges("da_similarity_nw_edges_long_begin", sequences, matrixName, gapOpen, gapExt, thresh_p)


def _thresh_args(thresh_p, threshold):
    """(thresh, thresh_is_quantile) of the *_cross_edges_begin calls: a threshold that is not None selects the absolute form"""
    return (float(thresh_p), 1) if threshold is None else (float(threshold), 0)


def similarityMH_cross_edges(x, y, k=4, n_hash=50, thresh_p=0.8, *, threshold=None, seed=None):
    """The entries of R = similarityMH_cross(x, y, k, n_hash, seed=seed) that pass a threshold, without the (m, n) matrix:
    ``(threshold, i, j, weight)`` with every (i, j) where ``R[i, j] >= threshold and R[i, j] > 0`` (clusterbreak's
    ``pep.sim[pep.sim < threshold] <- 0``; a zero weight is no edge), 0-based, sorted by (i, j) -- the order of ``np.nonzero`` -- and
    ``weight`` bit for bit ``R[i, j]``.  ``threshold=None``: the threshold is R's type-7 ``quantile(as.vector(R), thresh_p)`` over all
    m * n entries; a ``threshold`` that is not None is taken as it is (a range query: every y within that similarity of each x) and
    ``thresh_p`` is unused.  Errors as similarityMH_cross, then ``thresh_p`` outside [0, 1] / a NaN threshold."""
    lib, xr, xo, m, yr, yo, n, k, n_hash, seeds = _mh_prelude_two(x, y, k, n_hash, seed)
    thresh, is_q = _thresh_args(thresh_p, threshold)
    return _edges_one_pass(lambda h, thr, cnt: lib.da_similarity_mh_cross_edges_begin(
        xr.ctypes.data, xo.ctypes.data, m, yr.ctypes.data, yo.ctypes.data, n, k, n_hash, seeds.ctypes.data, thresh, is_q, h, thr, cnt))


def similarityMH_lsh_edges(sequences, k=4, n_hash=50, bands=10, rows=5, threshold=0.5, *, seed=None, max_candidates=1 << 32):
    """The threshold graph of one set from LSH candidates instead of all n (n - 1) / 2 pairs: ``(threshold, i, j, weight)``, 0-based, sorted
    by (i, j), the contract ``clusterbreak(edges_fn=)`` takes.  The signatures are cut into ``bands`` bands of ``rows`` hash functions
    (``bands * rows <= n_hash``; the columns behind belong to no band but count); two sequences are compared when some band agrees in all
    its columns.  The result is exactly ``lsh_edges_dense(minhash_signatures(sequences, k, n_hash, seed=seed), bands, rows, threshold)``:
    the diagonal at 1.0 and every candidate pair i < j with ``c / n_hash >= threshold`` (c = equal columns, the divide of similarityMH).
    What is approximate is that definition's relation to ``similarityMH_cross_edges(x, x, threshold=threshold)``: a pair above the
    threshold that agrees in no whole band is missing (``lsh_collision_probability`` says how likely).  ``max_candidates`` caps the
    (pair, band) incidences, which are known before any pair is compared: more raises DA_ERR_UNSUPPORTED."""
    lib, res, off, n, k, n_hash, seeds = _mh_prelude(sequences, k, n_hash, seed)
    bands, rows = _as_int(bands, "bands"), _as_int(rows, "rows")
    _thr, ei, ej, ew = _edges_one_pass(lambda h, _t, cnt: lib.da_similarity_mh_lsh_edges_begin(
        res.ctypes.data, off.ctypes.data, n, k, n_hash, seeds.ctypes.data, bands, rows, float(threshold), int(max_candidates), h, cnt))
    return float(threshold), ei, ej, ew


def mh_lsh_last_route():
    """What this thread's last LSH call did: buckets, (pair, band) incidences, distinct candidate pairs, edges (diagonal included)."""
    v = np.zeros(4, np.int64)
    _capi.check(_capi.load().da_mh_lsh_last_route(*[v[i:].ctypes.data for i in range(4)]))
    return dict(zip(("buckets", "incidences", "verified_pairs", "edges"), (int(x) for x in v)))


def lsh_edges_dense(sig, bands, rows, threshold):
    """The definition ``similarityMH_lsh_edges`` is exact against, in numpy (host code, the role of ``knn_dense`` / ``jaccard_dense``):
    ``sig`` is the (n, n_hash) uint32 signature matrix; -> ``(i, j, w)`` sorted by (i, j): (i, i, 1.0) for every i and (i, j, c / n_hash)
    for i < j that agree in all ``rows`` columns of some band and have ``c / n_hash >= threshold``."""
    sig = np.ascontiguousarray(sig, np.uint32)
    n, n_hash = sig.shape
    bands, rows = int(bands), int(rows)
    if bands < 1 or rows < 1 or bands * rows > n_hash:
        raise ValueError("need bands >= 1, rows >= 1 and bands * rows <= n_hash")
    pairs = [np.stack([np.arange(n, dtype=np.int64)] * 2, 1)]
    for t in range(bands):
        band = np.ascontiguousarray(sig[:, t * rows:(t + 1) * rows])
        _, inv = np.unique(band.view(np.dtype((np.void, 4 * rows))).ravel(), return_inverse=True)
        inv = inv.ravel()
        order = np.argsort(inv, kind="stable")
        ends = np.flatnonzero(np.r_[inv[order][1:] != inv[order][:-1], True]) + 1
        begin = 0
        for end in ends:
            if end - begin > 1:
                g = order[begin:end]
                a, b = np.triu_indices(len(g), 1)
                pairs.append(np.stack([g[a], g[b]], 1))
            begin = end
    p = np.unique(np.concatenate(pairs), axis=0)            # sorted by (i, j), each candidate once
    c = np.empty(len(p), np.int64)
    for b0 in range(0, len(p), 1 << 16):
        q = p[b0:b0 + (1 << 16)]
        c[b0:b0 + len(q)] = (sig[q[:, 0]] == sig[q[:, 1]]).sum(1)
    w = c.astype(np.float64) / np.float64(n_hash)
    keep = (p[:, 0] == p[:, 1]) | (w >= float(threshold))
    return p[keep, 0].astype(np.int32), p[keep, 1].astype(np.int32), w[keep]


def similarityMH_lsh_components(sequences, k=4, n_hash=50, bands=10, rows=5, threshold=0.5, *, seed=None, max_candidates=1 << 32):
    """The connected components of the graph `similarityMH_lsh_edges` returns for the same arguments -- everything that is transitively
    similar at the threshold: duplicate classes at 1.0, near-duplicate families at 0.9 -- as ``(membership int32[n], n_components)``, ids
    from 1 in order of first appearance.  Exactly ``lsh_components_dense(minhash_signatures(sequences, k, n_hash, seed=seed), bands, rows,
    threshold)``.  The edges are never emitted, sorted or copied: the kept candidate pairs go into a union-find on the device and n labels
    come back.  Errors as `similarityMH_lsh_edges`."""
    lib, res, off, n, k, n_hash, seeds = _mh_prelude(sequences, k, n_hash, seed)
    member = np.zeros(max(n, 1), np.int32)
    cnt = np.zeros(1, np.int64)
    _capi.check(lib.da_similarity_mh_lsh_components(res.ctypes.data, off.ctypes.data, n, k, n_hash, seeds.ctypes.data, _as_int(bands, "bands"),
                                                    _as_int(rows, "rows"), float(threshold), int(max_candidates), member.ctypes.data,
                                                    cnt.ctypes.data))
    return member[:n], int(cnt[0])


def lsh_components_dense(sig, bands, rows, threshold):
    """The definition ``similarityMH_lsh_components`` is exact against, in numpy: `clusterbreak.components_dense` on the edges of
    `lsh_edges_dense` -> ``(membership int32[n], n_components)``."""
    from .clusterbreak import components_dense
    i, j, _ = lsh_edges_dense(sig, bands, rows, threshold)
    return components_dense(np.asarray(sig).shape[0], i, j)


def similarityMH_lsh_knn(sequences, k=4, n_hash=50, bands=10, rows=5, top=10, *, threshold=0.0, seed=None, max_candidates=1 << 32):
    """Nearest-neighbour lists from LSH candidates instead of all n (n - 1) pairs: ``(idx, val)``, (n, top) int32 and (n, top) float64.
    Row i lists the first ``top`` of ``{j != i : i and j agree in all columns of some band, c / n_hash >= threshold}`` by c descending, then
    j ascending (c = equal columns, the divide of similarityMH); a row with fewer candidates is padded with ``idx = -1, val = 0.0``, and
    ``val > 0`` marks exactly the real entries.  The result is exactly ``lsh_knn_dense(minhash_signatures(sequences, k, n_hash, seed=seed),
    bands, rows, top, threshold)``.  What is approximate is that definition's relation to ``similarityMH_knn``: a true neighbour that
    agrees in no whole band is missing; with ``rows = 1, bands = n_hash`` the lists equal similarityMH_knn's wherever its value is > 0.
    ``top`` is in 1 .. 1024 and is NOT clamped to n - 1; n = 1 gives one row of padding.  Byte-identical sequences fill each other's lists
    at 1.0: pass distinct sequences.  ``max_candidates`` as in similarityMH_lsh_edges."""
    lib, res, off, n, k, n_hash, seeds = _mh_prelude(sequences, k, n_hash, seed)
    top = _as_int(top, "top")
    shape = (max(n, 1), min(max(top, 1), 1024))
    idx = np.empty(shape, np.int32)
    val = np.empty(shape, np.float64)
    _capi.check(lib.da_similarity_mh_lsh_knn(res.ctypes.data, off.ctypes.data, n, k, n_hash, seeds.ctypes.data, _as_int(bands, "bands"),
                                             _as_int(rows, "rows"), float(threshold), top, int(max_candidates), idx.ctypes.data, val.ctypes.data))
    return idx[:n], val[:n]


def similarityMH_lsh_knn_edges(sequences, k=4, n_hash=50, bands=10, rows=5, top=10, mode="union", *, threshold=0.0, seed=None,
                               max_candidates=1 << 32):
    """The kNN graph of similarityMH_lsh_knn as ``(threshold, i, j, w)`` for ``clusterbreak(edges_fn=)``: knn_graph of the lists (the
    padding has value 0 and is no edge) with the 1.0 diagonal of similarityMH.  The ``threshold`` slot holds the smallest off-diagonal
    weight kept, NaN when none."""
    idx, val = similarityMH_lsh_knn(sequences, k, n_hash, bands, rows, top, threshold=threshold, seed=seed, max_candidates=max_candidates)
    return _knn_edges_result(idx, val, 1.0, mode)


def lsh_knn_dense(sig, bands, rows, top, threshold=0.0):
    """The definition ``similarityMH_lsh_knn`` is exact against, in numpy (host code, beside ``lsh_edges_dense``): ``sig`` is the
    (n, n_hash) uint32 signature matrix; -> ``(idx, val)``, (n, top) int32 / float64: row i holds the first ``top`` candidates j != i with
    ``c / n_hash >= threshold`` by (c descending, j ascending), then ``-1`` / ``0.0``.  1 <= top <= 1024; not clamped to n - 1."""
    top = _as_int(top, "top")
    if not 1 <= top <= 1024:
        raise ValueError("top must be in 1 .. 1024 (got %d)" % top)
    ei, ej, w = lsh_edges_dense(sig, bands, rows, threshold)
    n, n_hash = np.asarray(sig).shape
    off = ei != ej
    ei, ej, w = ei[off].astype(np.int64), ej[off].astype(np.int64), w[off]
    r, c, v = np.concatenate([ei, ej]), np.concatenate([ej, ei]), np.concatenate([w, w])
    order = np.lexsort((c, -v, r))               # row, then value descending (= count descending: one divide), then column ascending
    r, c, v = r[order], c[order], v[order]
    start = np.searchsorted(r, np.arange(n))
    rank = np.arange(len(r)) - start[r]
    keep = rank < top
    idx = np.full((n, top), -1, np.int32)
    val = np.zeros((n, top), np.float64)
    idx[r[keep], rank[keep]] = c[keep]
    val[r[keep], rank[keep]] = v[keep]
    return idx, val


def similarityMH_lsh_cross_edges(x, y, k=4, n_hash=50, bands=10, rows=5, threshold=0.5, *, seed=None, max_candidates=1 << 32):
    """The threshold form of two sets from LSH candidates instead of all m * n pairs: ``(threshold, i, j, weight)``, 0-based, sorted by
    (i, j): every pair of an x[i] and a y[j] that agree in all columns of some band and have ``c / n_hash >= threshold`` (c = equal
    columns, the divide of similarityMH_cross).  No diagonal; every weight is > 0.  The result is exactly
    ``lsh_cross_edges_dense(minhash_signatures(x, ...), minhash_signatures(y, ...), bands, rows, threshold)``; approximate is only that
    definition's relation to ``similarityMH_cross_edges(x, y, threshold=threshold)``: a pair that agrees in no whole band is missing
    (``1 - lsh_collision_probability`` says how likely).  y is bucketed once (an index of its sorted band keys), x looks its keys up;
    ``MinHashSession.lsh_cross_edges`` keeps that index between calls.  ``max_candidates`` caps the (pair, band) incidences."""
    lib, xr, xo, m, yr, yo, n, k, n_hash, seeds = _mh_prelude_two(x, y, k, n_hash, seed)
    bands, rows = _as_int(bands, "bands"), _as_int(rows, "rows")
    thr, ei, ej, ew = _edges_one_pass(lambda h, _thr, cnt: lib.da_similarity_mh_lsh_cross_edges_begin(
        xr.ctypes.data, xo.ctypes.data, m, yr.ctypes.data, yo.ctypes.data, n, k, n_hash, seeds.ctypes.data, bands, rows, float(threshold),
        int(max_candidates), h, cnt))
    return float(threshold), ei, ej, ew


def similarityMH_lsh_cross_topk(x, y, k=4, n_hash=50, bands=10, rows=5, top=10, *, threshold=0.0, seed=None, max_candidates=1 << 32):
    """For every x[i] its ``top`` most similar y[j] among the LSH candidates: ``(idx, val)``, (m, top) int32 and (m, top) float64.  Row i
    lists the first ``top`` of ``{j : x[i] and y[j] agree in all columns of some band, c / n_hash >= threshold}`` by c descending, then j
    ascending; a row with fewer candidates is padded with ``idx = -1, val = 0.0`` and ``val > 0`` marks exactly the real entries.  ``top``
    is in 1 .. 1024 and is NOT clamped to len(y).  Exactly ``lsh_cross_topk_dense`` of the two signature matrices; with ``rows = 1, bands =
    n_hash`` the lists equal similarityMH_cross_topk's wherever its value is > 0.  ``max_candidates`` as in similarityMH_lsh_cross_edges."""
    lib, xr, xo, m, yr, yo, n, k, n_hash, seeds = _mh_prelude_two(x, y, k, n_hash, seed)
    top = _as_int(top, "top")
    shape = (max(m, 1), min(max(top, 1), 1024))
    idx = np.empty(shape, np.int32)
    val = np.empty(shape, np.float64)
    _capi.check(lib.da_similarity_mh_lsh_cross_topk(xr.ctypes.data, xo.ctypes.data, m, yr.ctypes.data, yo.ctypes.data, n, k, n_hash, seeds.ctypes.data,
                                                    _as_int(bands, "bands"), _as_int(rows, "rows"), float(threshold), top, int(max_candidates),
                                                    idx.ctypes.data, val.ctypes.data))
    return idx[:m], val[:m]


def lsh_cross_edges_dense(sig_x, sig_y, bands, rows, threshold):
    """The definition ``similarityMH_lsh_cross_edges`` is exact against, in numpy (host code, beside ``lsh_edges_dense``): ``sig_x`` (m,
    n_hash) and ``sig_y`` (n, n_hash) uint32 -> ``(i, j, w)`` sorted by (i, j): (i, j, c / n_hash) for every row i of sig_x and row j of
    sig_y that agree in all ``rows`` columns of some band and have ``c / n_hash >= threshold``."""
    sig_x, sig_y = np.ascontiguousarray(sig_x, np.uint32), np.ascontiguousarray(sig_y, np.uint32)
    (m, n_hash), (n, nh_y) = sig_x.shape, sig_y.shape
    bands, rows = int(bands), int(rows)
    if nh_y != n_hash:
        raise ValueError("sig_x and sig_y must have the same number of columns")
    if bands < 1 or rows < 1 or bands * rows > n_hash:
        raise ValueError("need bands >= 1, rows >= 1 and bands * rows <= n_hash")
    pairs = [np.empty((0, 2), np.int64)]
    void = np.dtype((np.void, 4 * rows))
    for t in range(bands):
        bx = np.ascontiguousarray(sig_x[:, t * rows:(t + 1) * rows]).view(void).ravel()
        by = np.ascontiguousarray(sig_y[:, t * rows:(t + 1) * rows]).view(void).ravel()
        _, inv = np.unique(np.concatenate([bx, by]), return_inverse=True)
        inv = inv.ravel()
        ix, iy = inv[:m], inv[m:]
        order = np.argsort(iy, kind="stable")                  # the rows of y by bucket
        sorted_y = iy[order]
        lo, hi = np.searchsorted(sorted_y, ix, "left"), np.searchsorted(sorted_y, ix, "right")
        ln = hi - lo
        if ln.sum():
            i = np.repeat(np.arange(m, dtype=np.int64), ln)
            within = np.arange(int(ln.sum()), dtype=np.int64) - np.repeat(np.cumsum(ln) - ln, ln)
            pairs.append(np.stack([i, order[np.repeat(lo, ln) + within].astype(np.int64)], 1))
    p = np.unique(np.concatenate(pairs), axis=0)               # sorted by (i, j), each candidate once
    c = np.empty(len(p), np.int64)
    for b0 in range(0, len(p), 1 << 16):
        q = p[b0:b0 + (1 << 16)]
        c[b0:b0 + len(q)] = (sig_x[q[:, 0]] == sig_y[q[:, 1]]).sum(1)
    w = c.astype(np.float64) / np.float64(n_hash)
    keep = w >= float(threshold)
    return p[keep, 0].astype(np.int32), p[keep, 1].astype(np.int32), w[keep]


def lsh_cross_topk_dense(sig_x, sig_y, bands, rows, top, threshold=0.0):
    """The definition ``similarityMH_lsh_cross_topk`` is exact against, in numpy: -> ``(idx, val)``, (m, top) int32 / float64: row i holds the
    first ``top`` candidates j of ``lsh_cross_edges_dense`` by (c descending, j ascending), then ``-1`` / ``0.0``.  1 <= top <= 1024; not
    clamped to the rows of sig_y."""
    top = _as_int(top, "top")
    if not 1 <= top <= 1024:
        raise ValueError("top must be in 1 .. 1024 (got %d)" % top)
    r, c, v = lsh_cross_edges_dense(sig_x, sig_y, bands, rows, threshold)
    m = np.asarray(sig_x).shape[0]
    r, c = r.astype(np.int64), c.astype(np.int64)
    order = np.lexsort((c, -v, r))               # row, then value descending (= count descending: one divide), then column ascending
    r, c, v = r[order], c[order], v[order]
    start = np.searchsorted(r, np.arange(m))
    rank = np.arange(len(r)) - start[r]
    keep = rank < top
    idx = np.full((m, top), -1, np.int32)
    val = np.zeros((m, top), np.float64)
    idx[r[keep], rank[keep]] = c[keep]
    val[r[keep], rank[keep]] = v[keep]
    return idx, val


def lsh_collision_probability(s, bands, rows):
    """P(two sequences of MinHash similarity ``s`` agree in at least one of ``bands`` bands of ``rows`` hash functions)
    = 1 - (1 - s^rows)^bands: the S-curve to choose bands and rows by."""
    s = np.asarray(s, np.float64)
    p = 1.0 - (1.0 - s ** int(rows)) ** int(bands)
    return float(p) if p.ndim == 0 else p


def similarityNW_lsh_edges(sequences, k=4, n_hash=50, bands=10, rows=5, threshold=0.5, *, mh_threshold=0.0, matrixName="BLOSUM62", gapOpen=10,
                           gapExt=4, seed=None, max_candidates=1 << 32):
    """The alignment-identity graph of one set at LSH cost: MinHash LSH chooses the pairs, Needleman-Wunsch scores them.
    ``(threshold, i, j, weight)``, 0-based, sorted by (i, j), the contract ``clusterbreak(edges_fn=)`` takes.  The candidates are the
    entries of ``similarityMH_lsh_edges(sequences, k, n_hash, bands, rows, mh_threshold, seed=seed)`` -- every (i, i) and every i < j that
    share a bucket and have ``c / n_hash >= mh_threshold``; each one, the diagonal included, is aligned (sequences[i] as sequence1) and kept
    when ``w = matches / length`` has ``w >= threshold and w > 0``.  The result is exactly ``nw_lsh_edges_dense`` of the signatures and the
    reference's pair value, weights bit for bit; approximate is only its relation to the all-pairs graph
    ``similarityNW_cross_edges_long(x, x, threshold=threshold)``: a pair that shares no bucket is missing.  Sequences of 1 .. 1024 residues,
    mixed freely; pass distinct strings.  Nothing returns to the host between bucketing and the final list.  Errors: the matrix name, then
    those of similarityMH_lsh_edges, then invalid residues, an empty sequence, one over 1024 residues, then the two thresholds."""
    lib, res, off, n, k, n_hash, seeds = _mh_prelude(sequences, k, n_hash, seed)
    name = _matrix_name(matrixName)
    go, ge = _as_int(gapOpen, "gapOpen"), _as_int(gapExt, "gapExt")
    bands, rows = _as_int(bands, "bands"), _as_int(rows, "rows")
    _thr, ei, ej, ew = _edges_one_pass(lambda h, _t, cnt: lib.da_similarity_nw_lsh_edges_begin(
        res.ctypes.data, off.ctypes.data, n, k, n_hash, seeds.ctypes.data, bands, rows, float(mh_threshold), int(max_candidates), name, go, ge,
        float(threshold), h, cnt))
    return float(threshold), ei, ej, ew


def similarityNW_lsh_cross_edges(x, y, k=4, n_hash=50, bands=10, rows=5, threshold=0.5, *, mh_threshold=0.0, matrixName="BLOSUM62", gapOpen=10,
                                 gapExt=4, seed=None, max_candidates=1 << 32):
    """The two-set form of ``similarityNW_lsh_edges``: the candidates of ``similarityMH_lsh_cross_edges(x, y, ..., mh_threshold)``, each
    aligned with x[i] as sequence1 and y[j] as sequence2, kept when ``w >= threshold and w > 0``.  No diagonal.  Exactly
    ``nw_lsh_cross_edges_dense`` of the two signature matrices and the reference's pair value."""
    lib, xr, xo, m, yr, yo, n, k, n_hash, seeds = _mh_prelude_two(x, y, k, n_hash, seed)
    name = _matrix_name(matrixName)
    go, ge = _as_int(gapOpen, "gapOpen"), _as_int(gapExt, "gapExt")
    bands, rows = _as_int(bands, "bands"), _as_int(rows, "rows")
    _thr, ei, ej, ew = _edges_one_pass(lambda h, _t, cnt: lib.da_similarity_nw_lsh_cross_edges_begin(
        xr.ctypes.data, xo.ctypes.data, m, yr.ctypes.data, yo.ctypes.data, n, k, n_hash, seeds.ctypes.data, bands, rows, float(mh_threshold),
        int(max_candidates), name, go, ge, float(threshold), h, cnt))
    return float(threshold), ei, ej, ew


def nw_lsh_last_route():
    """What this thread's last NW-on-LSH call did: buckets, (pair, band) incidences, distinct verified pairs, aligned pairs (the candidates,
    diagonal included), how many of them took the lane-per-pair (short) and the wavefront-per-pair (long) kernel, and edges -- after a
    list call (similarityNW_lsh_knn, similarityNW_lsh_cross_topk) the real list entries written."""
    v = np.zeros(7, np.int64)
    _capi.check(_capi.load().da_nw_lsh_last_route(*[v[i:].ctypes.data for i in range(7)]))
    return dict(zip(("buckets", "incidences", "verified_pairs", "aligned_pairs", "short_pairs", "long_pairs", "edges"), (int(x) for x in v)))


def _nw_threshold_keep(ci, cj, nw_value, threshold):
    w = np.array([nw_value(int(a), int(b)) for a, b in zip(ci, cj)], np.float64).reshape(-1)
    keep = (w >= float(threshold)) & (w > 0)
    return ci[keep], cj[keep], w[keep]


def nw_lsh_edges_dense(sig, bands, rows, mh_threshold, nw_value, threshold):
    """The definition ``similarityNW_lsh_edges`` is exact against (host code, beside ``lsh_edges_dense``): the candidates are exactly the
    pairs ``lsh_edges_dense(sig, bands, rows, mh_threshold)`` returns -- every (i, i), and every i < j that agree in a whole band and have
    ``c / n_hash >= mh_threshold``; ``nw_value(i, j)`` is the double ``matches / length`` of x[i] as sequence1 against x[j] as sequence2; a
    candidate is an edge when ``w = nw_value(i, j)`` has ``w >= threshold and w > 0``.  The diagonal is scored like every other pair.
    -> ``(i, j, w)`` sorted by (i, j)."""
    ci, cj, _ = lsh_edges_dense(sig, bands, rows, mh_threshold)
    return _nw_threshold_keep(ci, cj, nw_value, threshold)


def nw_lsh_cross_edges_dense(sig_x, sig_y, bands, rows, mh_threshold, nw_value, threshold):
    """The two-set twin of ``nw_lsh_edges_dense``: the candidates of ``lsh_cross_edges_dense(sig_x, sig_y, bands, rows, mh_threshold)``, no
    diagonal; ``nw_value(i, j)`` is x[i] as sequence1 against y[j] as sequence2."""
    ci, cj, _ = lsh_cross_edges_dense(sig_x, sig_y, bands, rows, mh_threshold)
    return _nw_threshold_keep(ci, cj, nw_value, threshold)


def _lsh_topk_arrays(rows_n, top):
    top = _as_int(top, "top")
    shape = (max(rows_n, 1), min(max(top, 1), 1024))
    return top, np.empty(shape, np.int32), np.empty(shape, np.float64)


def _nw_lsh_knn(sequences, k, n_hash, bands, rows, top, mh_threshold, threshold, matrixName, gapOpen, gapExt, seed, max_candidates):
    lib, res, off, n, k, n_hash, seeds = _mh_prelude(sequences, k, n_hash, seed)
    top, idx, val = _lsh_topk_arrays(n, top)
    diag = np.empty(max(n, 1), np.float64)
    _capi.check(lib.da_similarity_nw_lsh_knn(res.ctypes.data, off.ctypes.data, n, k, n_hash, seeds.ctypes.data, _as_int(bands, "bands"),
                                             _as_int(rows, "rows"), float(mh_threshold), int(max_candidates), _matrix_name(matrixName),
                                             _as_int(gapOpen, "gapOpen"), _as_int(gapExt, "gapExt"), float(threshold), top, idx.ctypes.data,
                                             val.ctypes.data, diag.ctypes.data))
    return idx[:n], val[:n], diag[:n]


def similarityNW_lsh_knn(sequences, k=4, n_hash=50, bands=10, rows=5, top=10, *, mh_threshold=0.0, threshold=0.0, matrixName="BLOSUM62",
                         gapOpen=10, gapExt=4, seed=None, max_candidates=1 << 32):
    """For every sequence its ``top`` best LSH candidates ranked by alignment identity: ``(idx, val)``, (n, top) int32 and (n, top) float64.
    The candidates are those of ``similarityNW_lsh_edges`` -- the pairs ``similarityMH_lsh_edges(..., mh_threshold)`` proposes -- each
    aligned once, the smaller position as sequence1 (the value similarityNW's symmetric matrix holds at both places).  Row r lists the
    first ``top`` of ``{c : {r, c} a candidate, w >= threshold and w > 0}`` by w descending, then c ascending; a row with fewer is padded
    with ``idx = -1, val = 0.0``, and ``val > 0`` marks exactly the real entries.  Equal doubles tie whatever their (matches, length).
    Exactly ``nw_lsh_knn_dense`` of the signatures and the reference's pair value, values bit for bit; approximate is only its relation
    to ``similarityNW_knn_long``: a neighbour that shares no bucket is missing.  Sequences of 1 .. 1024 residues, mixed freely; ``top`` is
    in 1 .. 1024 and is NOT clamped to n - 1.  The device orders 32-bit value ranks (``nw_value_ranks``); nothing but the lists returns to
    the host.  Errors as similarityNW_lsh_edges, ``top`` behind ``max_candidates`` with similarityMH_lsh_knn's text."""
    idx, val, _ = _nw_lsh_knn(sequences, k, n_hash, bands, rows, top, mh_threshold, threshold, matrixName, gapOpen, gapExt, seed, max_candidates)
    return idx, val


def similarityNW_lsh_knn_edges(sequences, k=4, n_hash=50, bands=10, rows=5, top=10, mode="union", *, mh_threshold=0.0, threshold=0.0,
                               matrixName="BLOSUM62", gapOpen=10, gapExt=4, seed=None, max_candidates=1 << 32):
    """The kNN graph of similarityNW_lsh_knn as ``(threshold, i, j, w)`` for ``clusterbreak(edges_fn=)``: knn_graph of the lists with the
    diagonal the DP gives for every sequence against itself (scored, not assumed to be 1.0).  At most ``n * top`` off-diagonal edges.  The
    ``threshold`` slot holds the smallest off-diagonal weight kept, NaN when none."""
    idx, val, diag = _nw_lsh_knn(sequences, k, n_hash, bands, rows, top, mh_threshold, threshold, matrixName, gapOpen, gapExt, seed, max_candidates)
    return _knn_edges_result(idx, val, diag, mode)


def similarityNW_lsh_cross_topk(x, y, k=4, n_hash=50, bands=10, rows=5, top=10, *, mh_threshold=0.0, threshold=0.0, matrixName="BLOSUM62",
                                gapOpen=10, gapExt=4, seed=None, max_candidates=1 << 32):
    """The two-set form of ``similarityNW_lsh_knn``: for every x[i] the first ``top`` of the candidates y[j] of
    ``similarityMH_lsh_cross_edges(x, y, ..., mh_threshold)`` by alignment identity (x[i] as sequence1, y[j] as sequence2) descending, then j
    ascending: ``(idx, val)``, (m, top).  No diagonal; ``top`` is NOT clamped to len(y).  Exactly ``nw_lsh_cross_topk_dense``."""
    lib, xr, xo, m, yr, yo, n, k, n_hash, seeds = _mh_prelude_two(x, y, k, n_hash, seed)
    top, idx, val = _lsh_topk_arrays(m, top)
    _capi.check(lib.da_similarity_nw_lsh_cross_topk(xr.ctypes.data, xo.ctypes.data, m, yr.ctypes.data, yo.ctypes.data, n, k, n_hash, seeds.ctypes.data,
                                                    _as_int(bands, "bands"), _as_int(rows, "rows"), float(mh_threshold), int(max_candidates),
                                                    _matrix_name(matrixName), _as_int(gapOpen, "gapOpen"), _as_int(gapExt, "gapExt"), float(threshold),
                                                    top, idx.ctypes.data, val.ctypes.data))
    return idx[:m], val[:m]


def _ranked_rows(r, c, w, n_rows, top, threshold):
    """the first ``top`` of every row's (c, w) with w >= threshold and w > 0 by (w descending, c ascending) -> (idx, val), padded -1 / 0.0"""
    top = _as_int(top, "top")
    if not 1 <= top <= 1024:
        raise ValueError("top must be in 1 .. 1024 (got %d)" % top)
    live = (w >= float(threshold)) & (w > 0)
    r, c, w = r[live], c[live], w[live]
    order = np.lexsort((c, -w, r))
    r, c, w = r[order], c[order], w[order]
    place = np.arange(len(r)) - np.searchsorted(r, np.arange(n_rows))[r]
    keep = place < top
    idx = np.full((n_rows, top), -1, np.int32)
    val = np.zeros((n_rows, top), np.float64)
    idx[r[keep], place[keep]] = c[keep]
    val[r[keep], place[keep]] = w[keep]
    return idx, val


def nw_lsh_knn_dense(sig, bands, rows, top, mh_threshold, nw_value, threshold=0.0):
    """The definition ``similarityNW_lsh_knn`` is exact against (host code, beside ``nw_lsh_edges_dense``) -> ``(idx, val, diag)``.  The
    candidates are the off-diagonal pairs i < j of ``lsh_edges_dense(sig, bands, rows, mh_threshold)``; ``w{i, j} = nw_value(i, j)``, the
    SMALLER position as sequence1 -- the value similarityNW's symmetric matrix holds at (i, j) and (j, i).  Row r lists the first ``top``
    (1 .. 1024, not clamped to n - 1) of ``{c : {r, c} a candidate, w >= threshold and w > 0}`` by w descending, then c ascending; the
    padding is -1 / 0.0.  ``diag[r] = nw_value(r, r)``.  Equal doubles tie whatever their (matches, length)."""
    ci, cj, _ = lsh_edges_dense(sig, bands, rows, mh_threshold)
    n = np.asarray(sig).shape[0]
    ci, cj = ci.astype(np.int64), cj.astype(np.int64)
    w = np.array([nw_value(int(a), int(b)) for a, b in zip(ci, cj)], np.float64).reshape(-1)
    diag = np.zeros(n, np.float64)
    on = ci == cj
    diag[ci[on]] = w[on]
    ci, cj, w = ci[~on], cj[~on], w[~on]
    idx, val = _ranked_rows(np.concatenate([ci, cj]), np.concatenate([cj, ci]), np.concatenate([w, w]), n, top, threshold)
    return idx, val, diag


def nw_lsh_cross_topk_dense(sig_x, sig_y, bands, rows, top, mh_threshold, nw_value, threshold=0.0):
    """The two-set twin of ``nw_lsh_knn_dense`` -> ``(idx, val)``: the candidates of ``lsh_cross_edges_dense(sig_x, sig_y, bands, rows,
    mh_threshold)``, ``nw_value(i, j)`` with x[i] as sequence1 and y[j] as sequence2; the rows are those of x, no diagonal."""
    ci, cj, _ = lsh_cross_edges_dense(sig_x, sig_y, bands, rows, mh_threshold)
    ci, cj = ci.astype(np.int64), cj.astype(np.int64)
    w = np.array([nw_value(int(a), int(b)) for a, b in zip(ci, cj)], np.float64).reshape(-1)
    return _ranked_rows(ci, cj, w, np.asarray(sig_x).shape[0], top, threshold)


def similarityNW_cross_edges(x, y, matrixName="BLOSUM62", gapOpen=10, gapExt=4, thresh_p=0.8, *, threshold=None):
    """The entries of R = similarityNW_cross(x, y, ...) (x[i] is sequence1) that pass a threshold: ``(threshold, i, j, weight)`` as
    similarityMH_cross_edges.  Equal similarities pass or fail together whatever their (matches, length): 2/4 and 3/6 are both 0.5.
    Every sequence has 1 .. 127 residues (an empty one is refused: a NaN has no place in a quantile).  An empty ``x`` or ``y`` gives no
    edges in the absolute form and is an error in the quantile form (an empty set has no quantile)."""
    return _nw_cross_edges("da_similarity_nw_cross_edges_begin", x, y, matrixName, gapOpen, gapExt, thresh_p, threshold)


def _nw_cross_edges(entry, x, y, matrixName, gapOpen, gapExt, thresh_p, threshold):
    lib = _capi.load()
    xr, xo, m, yr, yo, n = _pack_two(x, y)
    name = _matrix_name(matrixName)
    go, ge = _as_int(gapOpen, "gapOpen"), _as_int(gapExt, "gapExt")
    thresh, is_q = _thresh_args(thresh_p, threshold)
    return _edges_one_pass(lambda h, thr, cnt: getattr(lib, entry)(
        xr.ctypes.data, xo.ctypes.data, m, yr.ctypes.data, yo.ctypes.data, n, name, go, ge, thresh, is_q, h, thr, cnt))


def similarityNW_cross_edges_long(x, y, matrixName="BLOSUM62", gapOpen=10, gapExt=4, thresh_p=0.8, *, threshold=None):
    """``similarityNW_cross_edges`` for sequences of 1 .. 1024 residues (da_similarity_nw_cross_edges_long_begin): the same arguments, the
    same result, the same errors."""
    return _nw_cross_edges("da_similarity_nw_cross_edges_long_begin", x, y, matrixName, gapOpen, gapExt, thresh_p, threshold)


# ---- summary statistics (reference R/similarity.R:11-34) --------------------------------------------------------------------------------------

_STATS_FIELDS = ("mean_similarity", "median_similarity", "min_similarity", "max_similarity", "most_similar_pair", "least_similar_pair",
                 "most_similar_upper", "least_similar_upper")


class SimilarityStats(tuple):
    """The reference's ``similarity_stats`` list as a named tuple: ``mean_similarity``, ``median_similarity``, ``min_similarity``,
    ``max_similarity`` (floats) and ``most_similar_pair``, ``least_similar_pair`` -- R's ``which(X == v, arr.ind = TRUE)[1, ]`` as a 0-based
    ``(row, col)``: the first position in column-major order over the WHOLE matrix holding the extreme of the strict upper triangle, so
    ``(0, 0)`` when the maximum equals the diagonal -- plus two fields the reference lacks, ``most_similar_upper`` and
    ``least_similar_upper``: the first ``(i, j)`` with i < j in row-major order holding it."""
    __slots__ = ()
    _fields = _STATS_FIELDS

    def __new__(cls, *values):
        if len(values) != len(_STATS_FIELDS):
            raise TypeError("SimilarityStats takes %d values" % len(_STATS_FIELDS))
        return tuple.__new__(cls, values)

    def _asdict(self):
        return dict(zip(_STATS_FIELDS, self))

    def __repr__(self):
        return "SimilarityStats(%s)" % ", ".join("%s=%r" % kv for kv in zip(_STATS_FIELDS, self))


for _i, _name in enumerate(_STATS_FIELDS):
    setattr(SimilarityStats, _name, property(lambda self, _i=_i: self[_i]))
del _i, _name


def stats_from_histogram(hist, values):
    """(mean, median, min, max) of {values[b] repeated hist[b] times}, values ascending (da_stats_from_histogram): the median is R's /
    numpy's -- the plain average of the two middle elements for an even count -- and the mean one long double sum over the bins, within
    2 ** -42 relative of the exact mean of the doubles (not R's two-pass ``mean()`` bit for bit).  Needs no device."""
    lib = _capi.load()
    h = np.ascontiguousarray(hist, np.uint64)
    v = np.ascontiguousarray(values, np.float64)
    if h.shape != v.shape or h.ndim != 1:
        raise ValueError("hist and values must be one-dimensional and of one length")
    out = np.zeros(4, np.float64)
    _capi.check(lib.da_stats_from_histogram(h.ctypes.data, v.ctypes.data, len(h), out[0:].ctypes.data, out[1:].ctypes.data,
                                            out[2:].ctypes.data, out[3:].ctypes.data))
    return tuple(float(x) for x in out)


def compute_similarity_stats(X):
    """The reference's ``compute_similarity_stats`` (R/similarity.R:11-34) on a dense matrix, in numpy: mean, median, min and max of the strict
    upper triangle and the positions of the most and the least similar pair (``SimilarityStats``).  Its two checks: "Input must be a
    matrix" for anything but a two-dimensional array, and a warning when X is not symmetric.  The definitions are those of the device
    calls (``similarityMH_stats`` ...), which this function is what they are measured against: the median is ``np.median``'s, the mean
    the long double sum over the distinct values (``stats_from_histogram``).  A matrix without a strict upper triangle or with a NaN in
    it has no statistics here (ValueError); the reference returns NA for those and then fails on the subscript."""
    import warnings
    if not isinstance(X, np.ndarray) or X.ndim != 2:
        raise ValueError("Input must be a matrix")
    A = np.asarray(X, np.float64)
    rows, cols = A.shape
    eps100 = 100 * np.finfo(np.float64).eps                               # isSymmetric's tolerance
    if rows != cols or not (np.array_equal(A, A.T) or np.allclose(A, A.T, rtol=eps100, atol=0.0, equal_nan=True)):
        warnings.warn("Input matrix is not symmetric. Results may be unexpected.")
    U = np.concatenate([A[i, i + 1:] for i in range(min(rows, cols))]) if cols > 1 else np.zeros(0)   # the triangle without an index array
    if U.size == 0:
        raise ValueError("the matrix has no strict upper triangle: need >= 2 sequences")
    if np.isnan(U).any():
        raise ValueError("the strict upper triangle holds NaN")
    values, counts = np.unique(U, return_counts=True)
    mean, median, lo, hi = stats_from_histogram(counts, values)

    def first(v):
        c, r = divmod(int(np.argmax((A.T == v).ravel())), rows)           # column-major over the whole matrix: the first True of the transpose
        i, j = divmod(int(np.argmax(np.triu(A == v, 1).ravel())), cols)
        return (r, c), (i, j)
    most, most_upper = first(hi)
    least, least_upper = first(lo)
    return SimilarityStats(mean, median, lo, hi, most, least, most_upper, least_upper)


def _stats_result(s):
    """struct da_similarity_stats -> SimilarityStats"""
    return SimilarityStats(s.mean_similarity, s.median_similarity, s.min_similarity, s.max_similarity, tuple(s.most_similar_pair),
                           tuple(s.least_similar_pair), tuple(s.most_similar_upper), tuple(s.least_similar_upper))


def stats_from_records(hist, values, records):
    """``SimilarityStats`` from the two device passes over a resident n x n matrix of ranks: ``hist`` the histogram of its strict upper
    triangle over ``values`` (ascending, one per rank) and ``records`` the (n, 5) array of ``device.upper_extrema`` for the whole square
    (row_begin = col_begin = 0).  The host reduction of the C calls, in numpy."""
    rec = np.ascontiguousarray(records).view(np.uint32).reshape(-1, 5)
    mean, median, lo, hi = stats_from_histogram(hist, values)
    col = rec[:, [1, 3]].view(np.int32)
    has = col[:, 0] >= 0
    rows = np.arange(len(rec))
    out = []
    for want_max in (True, False):
        key, c = (rec[:, 2], col[:, 1]) if want_max else (rec[:, 0], col[:, 0])
        ext = key[has].max() if want_max else key[has].min()
        row_has = has & (key == ext)
        i = int(rows[row_has][0])
        upper = (i, int(c[i]))
        cand = row_has | (rec[:, 4] == ext)                               # rows ascending: the diagonal first, then the row's column
        r = int(rows[cand][0])
        pair = (r, r) if rec[r, 4] == ext else (int(c[r]), r)             # (c, r): column-major over the whole matrix, by symmetry
        if np.float64(values[int(ext)]) != (hi if want_max else lo):
            raise _capi.DynaAlignError(_capi.DA_ERR_HIP, "statistics mismatch between the histogram and the extrema pass")
        out += [pair, upper]
    return SimilarityStats(mean, median, lo, hi, out[0], out[2], out[1], out[3])


def similarityMH_stats(sequences, k=4, n_hash=50, *, seed=None):
    """``compute_similarity_stats(similarityMH(sequences, k, n_hash, seed=seed))`` without the matrix on the host: the uint16 counts stay on
    the device, a histogram of the strict upper triangle gives mean, median, min and max, and one more pass gives every row's extremes
    with their first columns, from which the positions follow (da_similarity_mh_stats).  Errors as similarityMH_edges."""
    lib, res, off, n, k, n_hash, seeds = _mh_prelude(sequences, k, n_hash, seed)
    s = _capi.DaSimilarityStats()
    _capi.check(lib.da_similarity_mh_stats(res.ctypes.data, off.ctypes.data, n, k, n_hash, seeds.ctypes.data, ctypes.addressof(s)))
    return _stats_result(s)


def _nw_stats(entry, sequences, matrixName, gapOpen, gapExt):
    lib = _capi.load()
    res, off = pack_sequences(sequences)
    n = len(off) - 1
    name = _matrix_name(matrixName)
    s = _capi.DaSimilarityStats()
    _capi.check(getattr(lib, entry)(res.ctypes.data, off.ctypes.data, n, name, _as_int(gapOpen, "gapOpen"), _as_int(gapExt, "gapExt"),
                                    ctypes.addressof(s)))
    return _stats_result(s)


def similarityNW_stats(sequences, matrixName="BLOSUM62", gapOpen=10, gapExt=4):
    """``compute_similarity_stats(similarityNW(sequences, ...))`` without the matrix on the host (da_similarity_nw_stats).  Equal similarities
    are one value whatever their (matches, length): 1/2 and 2/4 tie, for the median and for the positions.  The diagonal is what the
    alignment of a sequence with itself gives, not always 1.0.  Sequences of 1 .. 127 residues; errors as similarityNW_edges."""
    return _nw_stats("da_similarity_nw_stats", sequences, matrixName, gapOpen, gapExt)


def similarityNW_stats_long(sequences, matrixName="BLOSUM62", gapOpen=10, gapExt=4):
    """``similarityNW_stats`` for sequences of 1 .. 1024 residues (da_similarity_nw_stats_long): the same arguments, the same result, the same
    errors.  One pass of the alignment in row blocks, on 32-bit value ranks (``nw_value_ranks``)."""
    return _nw_stats("da_similarity_nw_stats_long", sequences, matrixName, gapOpen, gapExt)
