"""Device-resident front end: torch tensors in, torch tensors out.

PyTorch is plumbing here (HBM allocation, the current HIP stream,
torch.distributed); every computation is a launch of the library's HIP kernels
through the ``da_dev_*`` entry points of include/dynaalign.h.  Calls are
asynchronous on ``torch.cuda.current_stream()``.
"""
import ctypes

import numpy as np
import torch

from . import _capi
from ._capi import DA_OUT_COMPACT, DA_OUT_F64


def _call(fn, *args):
    """a library call that allocates on the device: when it runs out of memory, hand PyTorch's cached blocks back to the driver and try
    once more (the library's own out-of-memory path can only release its own parked buffers; a tensor PyTorch freed -- e.g. the count
    matrix MinHashSession reserves -- sits in PyTorch's allocator, invisible to hipMalloc)"""
    rc = fn(*args)
    if rc == _capi.DA_ERR_NOMEM:
        torch.cuda.empty_cache()
        rc = fn(*args)
    _capi.check(rc)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _require_cuda(t, name):
    if not t.is_cuda:
        raise _capi.DynaAlignError(_capi.DA_ERR_NO_DEVICE, "%s must live in HBM (dynaalign_amd has no CPU path)" % name)


def _seeds_tensor(seeds, device):
    """the hash seeds as the library takes them, uint32 words in an int32 device tensor: a tensor as it is, anything else through numpy"""
    if torch.is_tensor(seeds):
        return seeds
    return torch.from_numpy(np.ascontiguousarray(seeds, np.uint32).view(np.int32).copy()).to(device)


def _matrix_id(lib, matrix_name):
    mid = lib.da_matrix_id(matrix_name.encode("latin-1"))
    if mid < 0:
        _capi.check(_capi.DA_ERR_BAD_MATRIX)
    return mid


_WORK_TEXT = "work must be a contiguous uint8 tensor of %s bytes"


def _work(work, nbytes, device, error=None, flat=False, at_least=0):
    """The workspace of a call: the caller's tensor, or a new one of ``nbytes`` bytes (a number, or a function asked only then) when
    there is none.  ``error``, the exception to raise, makes it checked: in HBM, uint8, contiguous (``flat``: of one dimension with unit
    stride, whatever its address or length) and of at least ``at_least`` bytes.  Without it the tensor is taken as it is."""
    if work is None:
        work = torch.empty(nbytes() if callable(nbytes) else nbytes, dtype=torch.uint8, device=device)
    if error is not None:
        _require_cuda(work, "work")
        laid_out = (work.dim() == 1 and work.stride(0) == 1) if flat else work.is_contiguous()
        if work.dtype != torch.uint8 or not laid_out or int(work.numel()) < at_least:
            raise error
    return work


def _top(top):
    """the columns of a top-k result: `top`, at least one slot and at most the DA_TOPK_MAX the kernels select"""
    return max(min(int(top), _capi.DA_TOPK_MAX), 1)


def _topk_out(rows, top, key_dtype, device):
    """(idx int32, key or val of key_dtype), both (max(rows, 1), _top(top)) and unwritten"""
    shape = (max(rows, 1), _top(top))
    return torch.empty(shape, dtype=torch.int32, device=device), torch.empty(shape, dtype=key_dtype, device=device)


def _edge_slots(capacity, device, dtypes):
    """one unwritten tensor of max(capacity, 1) slots per dtype: the columns of an edge or entry list"""
    return tuple(torch.empty(max(capacity, 1), dtype=dt, device=device) for dt in dtypes)


def _count_then_fill(run, capacity, device, dtypes):
    """The capacity protocol of the LSH list calls.  ``run(cap, *pointers)`` makes the library call and returns the full number of
    entries.  capacity=None: a first call with capacity 0 and NULL columns counts, a second one fills; an int: the one call stores at
    most that many.  Returns the columns cut to what was stored."""
    if capacity is None:
        capacity = run(0, *[None] * len(dtypes))
    capacity = int(capacity)
    out = _edge_slots(capacity, device, dtypes)
    stored = min(run(capacity, *[t.data_ptr() for t in out]), capacity)
    return tuple(t[:stored] for t in out)


class DeviceSequences:
    """Packed sequences resident in HBM: residues uint8[total], offsets int64[n+1]."""

    def __init__(self, residues, offsets, device="cuda"):
        offsets = np.ascontiguousarray(offsets, np.int64)
        self.n = len(offsets) - 1
        self.total = int(offsets[-1]) if self.n >= 0 else 0
        lens = np.diff(offsets) if self.n > 0 else np.zeros(0, np.int64)
        self.max_len = int(lens.max()) if self.n > 0 else 0
        self.offsets_host = offsets
        res = np.ascontiguousarray(residues, np.uint8)[:max(self.total, 1)]
        self.residues = torch.from_numpy(res.copy()).to(device)
        self.offsets = torch.from_numpy(offsets.copy()).to(device)
        self.codes = None  # filled by nw_encode


def sig_ld(n_hash):
    return int(_capi.load().da_sig_ld(int(n_hash)))


def planes_words(n, n_hash):
    return int(_capi.load().da_mh_planes_words(int(n), int(n_hash)))


class Planes:
    """Operand of mh_compare: the (opaque, blocked) bit-plane buffer plus the number of planes it holds per
    group of 32 hash functions (8 / 12 / 16: dictionary codes from da_dev_mh_planes, 32: raw signature bits)."""

    def __init__(self, tensor, bits):
        self.tensor, self.bits = tensor, int(bits)

    def data_ptr(self):
        return self.tensor.data_ptr()

    @property
    def device(self):
        return self.tensor.device

    @property
    def is_cuda(self):
        return self.tensor.is_cuda


def planes_workspace_bytes(n, n_hash):
    return int(_capi.load().da_mh_planes_workspace_bytes(int(n), int(n_hash)))


def minhash_signatures(ds, k, n_hash, seeds, out=None, planes=None, want_planes=True, raw_planes=False, work=None,
                       min_plane_bits=0):
    """K1 (+ K1b).  Returns (sig, planes): `sig` is the int32 tensor (n, sig_ld(n_hash)) holding the uint32
    signatures in columns [0, n_hash); `planes` is the Planes operand of mh_compare (None if want_planes is
    False), see mh_planes.  raw_planes=True is min_plane_bits=32."""
    lib = _capi.load()
    seeds = _seeds_tensor(seeds, ds.residues.device)
    _require_cuda(ds.residues, "residues")
    ld = sig_ld(n_hash) if n_hash > 0 else 32
    if out is None:
        out = torch.empty((max(ds.n, 1), ld), dtype=torch.int32, device=ds.residues.device)
    _call(lib.da_dev_minhash_signatures, ds.residues.data_ptr(), ds.offsets.data_ptr(), ds.n, ds.total,
                                              ds.max_len, int(k), int(n_hash), seeds.data_ptr(), out.data_ptr(),
                                              out.stride(0), _stream())
    if not want_planes and planes is None:
        return out, None
    return out, mh_planes(out, ds.n, n_hash, planes, work, 32 if raw_planes else min_plane_bits)


def mh_planes(sig, n, n_hash, planes=None, work=None, min_plane_bits=0):
    """K1b.  Signature tensor -> Planes operand: the signatures' exact dictionary codes, bit-transposed, with
    8 / 12 / 16 planes per 32 hash functions (as few as the data needs, at least min_plane_bits) when
    n <= 131068; raw 32 planes otherwise or with min_plane_bits=32.  Synchronises the current stream once on
    the dictionary route.  `planes` / `work` may be preallocated: planes_words(n, n_hash) int32 and
    planes_workspace_bytes(n, n_hash) uint8."""
    lib = _capi.load()
    _require_cuda(sig, "signatures")
    if isinstance(planes, Planes):
        planes = planes.tensor
    if planes is None:
        planes = torch.empty(max(planes_words(n, n_hash), 4), dtype=torch.int32, device=sig.device)
    work = _work(work, lambda: planes_workspace_bytes(n, n_hash), sig.device)
    bits = ctypes.c_int(0)
    _call(lib.da_dev_mh_planes, sig.data_ptr(), sig.stride(0), n, int(n_hash), int(min_plane_bits),
                                     work.data_ptr(), work.numel(), planes.data_ptr(), planes.numel(),
                                     ctypes.byref(bits), _stream())
    return Planes(planes, bits.value)


def _alloc_out(rows, n, kind, device, out):
    if out is not None:
        return out
    dt = torch.float64 if kind == DA_OUT_F64 else torch.int16  # int16 holds the uint16 bit pattern
    try:
        return torch.empty((max(rows, 1), max(n, 1)), dtype=dt, device=device)
    except torch.OutOfMemoryError:
        # buffers the library parked for its next call are invisible to torch's allocator: hand them back and try once more
        torch.cuda.empty_cache()
        _capi.load().da_release_device_memory()
        return torch.empty((max(rows, 1), max(n, 1)), dtype=dt, device=device)


def mh_compare(planes, n, n_hash, row_begin=0, row_end=None, symmetric=None, kind=DA_OUT_F64, out=None):
    """K2.  `planes` is the Planes operand from minhash_signatures.  Rows [row_begin,row_end) of the
    n x n similarity (float64) or match-count (uint16 in an int16 tensor) matrix."""
    lib = _capi.load()
    _require_cuda(planes, "bit planes")
    row_end = n if row_end is None else row_end
    if symmetric is None:
        symmetric = (row_begin == 0 and row_end == n)
    out = _alloc_out(row_end - row_begin, n, kind, planes.device, out)
    _call(lib.da_dev_mh_compare, planes.data_ptr(), planes.bits, n, int(n_hash), row_begin,
                                      row_end, 1 if symmetric else 0, kind, out.data_ptr(), out.stride(0), _stream())
    return out


def mh_compare_rect(planes, n, n_hash, row_begin, row_end, col_begin, col_end, kind=DA_OUT_F64, out=None):
    """K2 on a rectangle: rows [row_begin, row_end) x columns [col_begin, col_end) of the n-row problem `planes` was built
    for, every element once (da_dev_mh_compare_rect).  Two sets are compared through ONE operand built on their
    concatenation; origins that are multiples of 128 get the hand-scheduled kernels."""
    lib = _capi.load()
    _require_cuda(planes, "bit planes")
    out = _alloc_out(row_end - row_begin, col_end - col_begin, kind, planes.device, out)
    _call(lib.da_dev_mh_compare_rect, planes.data_ptr(), planes.bits, int(n), int(n_hash), int(row_begin), int(row_end),
                                           int(col_begin), int(col_end), kind, out.data_ptr(), out.stride(0), _stream())
    return out


def nw_encode(ds):
    """K0.  Fills ds.codes; returns the int32 flag tensor (0 = all residues valid)."""
    lib = _capi.load()
    _require_cuda(ds.residues, "residues")
    ds.codes = torch.empty_like(ds.residues)
    bad = torch.zeros(1, dtype=torch.int32, device=ds.residues.device)
    _call(lib.da_dev_nw_encode, ds.residues.data_ptr(), ds.total, ds.codes.data_ptr(), bad.data_ptr(), _stream())
    return bad


def decode_bad_position(flag_value):
    """int from nw_encode's flag -> byte position of the first invalid residue, or None."""
    return None if flag_value == 0 else (2 ** 31 - 1) - int(flag_value)


def nw(ds, matrix_name="BLOSUM62", gap_open=10, gap_ext=4, row_begin=0, row_end=None, symmetric=None,
       kind=DA_OUT_F64, out=None, score=None):
    """K3.  ds.codes must be filled (nw_encode)."""
    lib = _capi.load()
    if ds.codes is None:
        raise ValueError("call nw_encode(ds) first")
    mid = _matrix_id(lib, matrix_name)
    n = ds.n
    row_end = n if row_end is None else row_end
    if symmetric is None:
        symmetric = (row_begin == 0 and row_end == n)
    out = _alloc_out(row_end - row_begin, n, kind, ds.residues.device, out)
    _call(lib.da_dev_nw, ds.codes.data_ptr(), ds.offsets.data_ptr(), n, ds.max_len, mid, int(gap_open),
                              int(gap_ext), row_begin, row_end, 1 if symmetric else 0, kind, out.data_ptr(),
                              out.stride(0), None if score is None else score.data_ptr(),
                              0 if score is None else score.stride(0), _stream())
    return out


def nw_rect(ds, matrix_name="BLOSUM62", gap_open=10, gap_ext=4, row_begin=0, row_end=None, col_begin=0, col_end=None,
            kind=DA_OUT_F64, out=None):
    """K3 on a rectangle (da_dev_nw_rect): element (i, j) = calc(seq[min(i, j)], seq[max(i, j)]).  On the codes of x + y,
    rows of x against columns of y give calc(x[i], y[j]); rows of y against columns of x its transpose."""
    lib = _capi.load()
    if ds.codes is None:
        raise ValueError("call nw_encode(ds) first")
    mid = _matrix_id(lib, matrix_name)
    n = ds.n
    row_end = n if row_end is None else row_end
    col_end = n if col_end is None else col_end
    if out is None:
        dt = {DA_OUT_F64: torch.float64, DA_OUT_COMPACT: torch.int16}.get(kind, torch.int32)
        out = torch.empty((max(row_end - row_begin, 1), max(col_end - col_begin, 1)), dtype=dt, device=ds.residues.device)
    _call(lib.da_dev_nw_rect, ds.codes.data_ptr(), ds.offsets.data_ptr(), n, ds.max_len, mid, int(gap_open), int(gap_ext),
                                   int(row_begin), int(row_end), int(col_begin), int(col_end), kind, out.data_ptr(), out.stride(0),
                                   _stream())
    return out


class JaccardSets:
    """Operand of jaccard_rect: per sequence the ascending distinct keys of its k-shingles -- ``keys`` (n, ld_keys), int32 for k <= 4 and int64
    for k 5 .. 8, holding the unsigned bit patterns of the k bytes packed big-endian -- and ``counts`` (n,) uint8, how many of a row's keys are
    its set (jaccard_sets_long: uint16 bit patterns in an int16 tensor, the operand of jaccard_rect_long); the rest of a row is zero and means
    nothing."""

    def __init__(self, keys, counts, n, k):
        self.keys, self.counts, self.n, self.k = keys, counts, int(n), int(k)

    @property
    def ld_keys(self):
        return self.keys.stride(0)


def jaccard_sets_ld(max_len, k):
    return int(_capi.load().da_dev_jaccard_sets_ld(int(max_len), int(k)))


def _jaccard_sets(entry, ld_of, count_dtype, ds, k):
    _require_cuda(ds.residues, "residues")
    k = int(k)
    ld = max(ld_of(ds.max_len, k), 4)
    keys = torch.empty((max(ds.n, 1), ld), dtype=torch.int32 if k <= 4 else torch.int64, device=ds.residues.device)
    counts = torch.empty(max(ds.n, 1), dtype=count_dtype, device=ds.residues.device)
    _call(entry, ds.residues.data_ptr(), ds.offsets.data_ptr(), ds.n, ds.max_len, k, keys.data_ptr(), ld, counts.data_ptr(), _stream())
    return JaccardSets(keys, counts, ds.n, k)


def _jaccard_rect(entry, code_dtype, sets, row_begin, row_end, col_begin, col_end, kind, out):
    _require_cuda(sets.keys, "shingle sets")
    n = sets.n
    row_end = n if row_end is None else row_end
    col_end = n if col_end is None else col_end
    if out is None:
        out = torch.empty((max(row_end - row_begin, 1), max(col_end - col_begin, 1)), dtype=torch.float64 if kind == DA_OUT_F64 else code_dtype,
                          device=sets.keys.device)
    _call(entry, sets.keys.data_ptr(), sets.counts.data_ptr(), n, sets.ld_keys, sets.k, int(row_begin), int(row_end), int(col_begin), int(col_end),
          kind, out.data_ptr(), out.stride(0), _stream())
    return out


def jaccard_sets(ds, k):
    """The shingle sets of the sequences in ``ds`` (da_dev_jaccard_sets): k in 1 .. 8, every sequence at most 127 shingle positions."""
    return _jaccard_sets(_capi.load().da_dev_jaccard_sets, jaccard_sets_ld, torch.uint8, ds, k)


def jaccard_rect(sets, row_begin=0, row_end=None, col_begin=0, col_end=None, kind=DA_OUT_F64, out=None):
    """The exact Jaccard index on a rectangle (da_dev_jaccard_rect): rows [row_begin, row_end) x columns [col_begin, col_end) of the sets, as
    float64 or as uint16 codes ``intersection << 8 | union`` in an int16 tensor.  On the sets of x + y, rows of x against columns of y give the
    two-set matrix.  ``out`` may be any view with unit column stride (its row stride is the leading dimension)."""
    return _jaccard_rect(_capi.load().da_dev_jaccard_rect, torch.int16, sets, row_begin, row_end, col_begin, col_end, kind, out)


def jaccard_sets_long_ld(max_len, k):
    return int(_capi.load().da_jaccard_sets_long_ld(int(max_len), int(k)))


def jaccard_sets_long(ds, k):
    """The shingle sets of the sequences in ``ds`` for up to 1024 shingle positions a sequence (da_dev_jaccard_sets_long): a JaccardSets whose
    ``counts`` are uint16 bit patterns in an int16 tensor, the operand of jaccard_rect_long."""
    return _jaccard_sets(_capi.load().da_dev_jaccard_sets_long, jaccard_sets_long_ld, torch.int16, ds, k)


def jaccard_rect_long(sets, row_begin=0, row_end=None, col_begin=0, col_end=None, kind=DA_OUT_F64, out=None):
    """The exact Jaccard index on a rectangle of the sets of jaccard_sets_long (da_dev_jaccard_rect_long): as jaccard_rect, with ``kind``
    DA_OUT_F64 or DA_OUT_PACK32 -- uint32 codes ``intersection << 16 | union`` (``1 << 16 | 1`` for two empty sets) in an int32 tensor.  A
    rectangle whose rows and columns are the same range is computed by the symmetric form."""
    return _jaccard_rect(_capi.load().da_dev_jaccard_rect_long, torch.int32, sets, row_begin, row_end, col_begin, col_end, kind, out)


class LevMasks:
    """Operand of lev_rect: ``masks``, one uint8 tensor of da_dev_lev_masks_bytes(n, max_len, n_classes) bytes holding per sequence the match
    masks of its classes, the class ids of its bytes and its length; ``class_map`` (256 uint8 on the host) numbers the bytes that occur as
    classes 0 .. n_classes - 1."""

    def __init__(self, masks, n, max_len, class_map, n_classes):
        self.masks, self.n, self.max_len, self.class_map, self.n_classes = masks, int(n), int(max_len), class_map, int(n_classes)


def lev_masks_bytes(n, max_len, n_classes):
    return int(_capi.load().da_dev_lev_masks_bytes(int(n), int(max_len), int(n_classes)))


def lev_masks(ds, class_map=None):
    """The match masks of the sequences in ``ds`` (da_dev_lev_masks): every sequence at most 127 bytes.  ``class_map``: 256 class ids, one per
    byte value; None numbers the byte values that occur in ``ds`` in ascending order, read from a host copy of the residues."""
    _require_cuda(ds.residues, "residues")
    if class_map is None:
        seen = np.zeros(256, bool)
        seen[np.unique(ds.residues[:ds.total].cpu().numpy())] = True
        class_map = np.where(seen, np.cumsum(seen) - 1, 0).astype(np.uint8)
    class_map = np.ascontiguousarray(class_map, np.uint8)
    if class_map.shape != (256,):
        raise ValueError("class_map must hold 256 class ids")
    n_classes = int(class_map.max()) + 1
    masks = torch.empty(max(lev_masks_bytes(ds.n, ds.max_len, n_classes), 8), dtype=torch.uint8, device=ds.residues.device)
    _call(_capi.load().da_dev_lev_masks, ds.residues.data_ptr(), ds.offsets.data_ptr(), ds.n, ds.max_len, class_map.ctypes.data, n_classes,
          masks.data_ptr(), masks.numel(), _stream())
    return LevMasks(masks, ds.n, ds.max_len, class_map, n_classes)


def lev_rect(masks, row_begin=0, row_end=None, col_begin=0, col_end=None, kind=DA_OUT_F64, out=None):
    """The Levenshtein similarity on a rectangle (da_dev_lev_rect): rows [row_begin, row_end) x columns [col_begin, col_end) of the operand of
    lev_masks, as float64 or as uint16 codes ``(L - d) << 8 | L`` in an int16 tensor.  On the masks of x + y, rows of x against columns of y
    give the two-set matrix; a rectangle whose rows and columns are the same range is computed by the symmetric form.  ``out`` may be any
    view with unit column stride (its row stride is the leading dimension)."""
    _require_cuda(masks.masks, "match masks")
    n = masks.n
    row_end = n if row_end is None else row_end
    col_end = n if col_end is None else col_end
    if out is None:
        out = torch.empty((max(row_end - row_begin, 1), max(col_end - col_begin, 1)), dtype=torch.float64 if kind == DA_OUT_F64 else torch.int16,
                          device=masks.masks.device)
    _call(_capi.load().da_dev_lev_rect, masks.masks.data_ptr(), n, masks.max_len, masks.n_classes, int(row_begin), int(row_end), int(col_begin),
          int(col_end), kind, out.data_ptr(), out.stride(0), _stream())
    return out


def nw_align_workspace_bytes(pairs):
    return int(_capi.load().da_nw_align_workspace_bytes(int(pairs)))


def nw_align_pairs(dx, dy, matrix_name="BLOSUM62", gap_open=10, gap_ext=4, pair_x=None, pair_y=None, ops=True, ld_ops=None, work=None):
    """The alignment paths of listed pairs on the device (da_dev_nw_align_pairs): pair p aligns dx[pair_x[p]] as sequence1 with
    dy[pair_y[p]] as sequence2; without lists pair p is dx[p] with dy[p].  dx.codes / dy.codes must be filled (nw_encode; dx may be dy);
    pair_x / pair_y: int32 device tensors.  Returns ``(ops, length, matches, score)``: ops a (pairs, ld_ops) uint8 tensor of 'D' / 'U' /
    'L' bytes, 0 past a row's length (None with ops=False), the others int32 tensors.  ld_ops defaults to dx.max_len + dy.max_len.
    Nothing is checked against the lists here: a pair the kernel cannot take (an index outside its set, more than 127 residues) gets
    length -1.  work: a uint8 device tensor of at least nw_align_workspace_bytes(64) bytes (allocated if None)."""
    lib = _capi.load()
    mid, pair_x, pair_y, pairs = _align_operands(lib, dx, dy, matrix_name, pair_x, pair_y)
    ld_ops, ops_t, ln, mt, sc = _align_out(dx, dy, pairs, ops, ld_ops)
    work = _work(work, lambda: max(nw_align_workspace_bytes(min(max(pairs, 64), 1 << 19)), 16), dx.residues.device)
    _call(lib.da_dev_nw_align_pairs, dx.codes.data_ptr(), dx.offsets.data_ptr(), dx.n, dy.codes.data_ptr(), dy.offsets.data_ptr(), dy.n,
          None if pair_x is None else pair_x.data_ptr(), None if pair_y is None else pair_y.data_ptr(), pairs, mid, int(gap_open), int(gap_ext),
          None if ops_t is None else ops_t.data_ptr(), ld_ops, ln.data_ptr(), mt.data_ptr(), sc.data_ptr(), work.data_ptr(),
          work.numel(), _stream())
    return (None if ops_t is None else ops_t[:pairs]), ln[:pairs], mt[:pairs], sc[:pairs]


def _align_operands(lib, dx, dy, matrix_name, pair_x, pair_y):
    """the checks nw_align_pairs and nw_align_long_pairs share, in their order -> (matrix id, pair_x, pair_y, number of pairs)"""
    if dx.codes is None or dy.codes is None:
        raise ValueError("call nw_encode on both sets first")
    mid = _matrix_id(lib, matrix_name)
    if (pair_x is None) != (pair_y is None):
        raise ValueError("pair_x and pair_y must both be given or both be None")
    if pair_x is None:
        if dx.n != dy.n:
            raise ValueError("without pair lists, dx and dy must hold the same number of sequences (got %d and %d)" % (dx.n, dy.n))
        return mid, None, None, dx.n
    _require_cuda(pair_x, "pair_x")
    _require_cuda(pair_y, "pair_y")
    if pair_x.dtype != torch.int32 or pair_y.dtype != torch.int32 or pair_x.numel() != pair_y.numel():
        raise ValueError("pair_x and pair_y must be int32 tensors of the same length")
    return mid, pair_x.contiguous(), pair_y.contiguous(), pair_x.numel()


def _align_out(dx, dy, pairs, ops, ld_ops):
    """-> (ld_ops, the ops rows or None, length, matches, score) of an alignment call, unwritten"""
    dev = dx.residues.device
    ld_ops = int(max(dx.max_len + dy.max_len, 1) if ld_ops is None else ld_ops)
    ops_t = torch.empty((max(pairs, 1), ld_ops), dtype=torch.uint8, device=dev) if ops else None
    ln = torch.empty(max(pairs, 1), dtype=torch.int32, device=dev)
    return ld_ops, ops_t, ln, torch.empty_like(ln), torch.empty_like(ln)


def nw_align_long_workspace_bytes(pairs, max_len):
    return int(_capi.load().da_nw_align_long_workspace_bytes(int(pairs), int(max_len)))


def nw_align_long_pairs(dx, dy, matrix_name="BLOSUM62", gap_open=10, gap_ext=4, pair_x=None, pair_y=None, ops=True, ld_ops=None, max_len=None,
                        work=None):
    """``nw_align_pairs`` for sequences of up to 1024 residues (da_dev_nw_align_long_pairs): one wavefront per pair, every pair, short
    ones included.  Arguments and result as ``nw_align_pairs``.  max_len sizes the slots of the workspace (None: the longest sequence of
    the two sets, from their offsets); a pair with a sequence over max_len, over 1024 residues, an index outside its set or
    ld_ops < len(x) + len(y) gets length -1.  work: a uint8 device tensor of at least nw_align_long_workspace_bytes(1, max_len) bytes
    (allocated if None; a smaller one than nw_align_long_workspace_bytes(pairs, max_len) means fewer wavefronts in flight); not needed
    with ops=False."""
    lib = _capi.load()
    mid, pair_x, pair_y, pairs = _align_operands(lib, dx, dy, matrix_name, pair_x, pair_y)
    max_len = max(int(dx.max_len), int(dy.max_len)) if max_len is None else int(max_len)
    ld_ops, ops_t, ln, mt, sc = _align_out(dx, dy, pairs, ops, ld_ops)
    if ops:
        work = _work(work, lambda: max(nw_align_long_workspace_bytes(pairs, max_len), 16), dx.residues.device)
    _call(lib.da_dev_nw_align_long_pairs, dx.codes.data_ptr(), dx.offsets.data_ptr(), dx.n, dy.codes.data_ptr(), dy.offsets.data_ptr(), dy.n,
          None if pair_x is None else pair_x.data_ptr(), None if pair_y is None else pair_y.data_ptr(), pairs, mid, int(gap_open), int(gap_ext),
          None if ops_t is None else ops_t.data_ptr(), ld_ops, ln.data_ptr(), mt.data_ptr(), sc.data_ptr(), max_len,
          None if work is None else work.data_ptr(), 0 if work is None else work.numel(), _stream())
    return (None if ops_t is None else ops_t[:pairs]), ln[:pairs], mt[:pairs], sc[:pairs]


def _cluster_table(cluster_ptr, device):
    """-> (host int64 array, device int64 tensor) of a pooled cluster table"""
    if isinstance(cluster_ptr, torch.Tensor):
        host = np.ascontiguousarray(cluster_ptr.detach().cpu().numpy(), np.int64)
    else:
        host = np.ascontiguousarray(cluster_ptr, np.int64)
    if host.ndim != 1 or len(host) < 1:
        raise ValueError("cluster_ptr must hold clusters + 1 entries")
    return host, torch.from_numpy(host.copy()).to(device)


def cluster_consensus_workspace_bytes(cluster_ptr, max_len, minimal=False):
    host = np.ascontiguousarray(cluster_ptr, np.int64)
    return int(_capi.load().da_dev_cluster_consensus_workspace_bytes(host.ctypes.data, len(host) - 1, int(max_len), int(bool(minimal))))


def cluster_consensus(ds, cluster_ptr, matrix_name="BLOSUM62", gap_open=10, gap_ext=4, work=None):
    """The center-star consensus of pooled clusters on the device (da_dev_cluster_consensus): cluster k is the sequences
    ds[cluster_ptr[k] : cluster_ptr[k + 1]], at least one each; ds.codes must be filled (nw_encode) and every residue valid.  Returns
    ``(cons, cons_len, center)``: a (clusters, max(ds.max_len, 1)) uint8 tensor of letters (bytes past a row's length are not written),
    the int32 lengths and the int32 pooled index of each cluster's center.  Asynchronous; nothing returns to the host between the
    center choice and the column vote.  work: a uint8 device tensor of at least cluster_consensus_workspace_bytes(cluster_ptr,
    ds.max_len, minimal=True) bytes (allocated at the size of the largest blocks if None)."""
    lib = _capi.load()
    if ds.codes is None:
        raise ValueError("call nw_encode first")
    mid = _matrix_id(lib, matrix_name)
    dev = ds.residues.device
    host, dptr = _cluster_table(cluster_ptr, dev)
    clusters = len(host) - 1
    ld = max(int(ds.max_len), 1)
    cons = torch.zeros((max(clusters, 1), ld), dtype=torch.uint8, device=dev)
    cons_len = torch.zeros(max(clusters, 1), dtype=torch.int32, device=dev)
    center = torch.zeros(max(clusters, 1), dtype=torch.int32, device=dev)
    work = _work(work, lambda: max(cluster_consensus_workspace_bytes(host, ds.max_len), 16), dev)
    _call(lib.da_dev_cluster_consensus, ds.codes.data_ptr(), ds.offsets.data_ptr(), ds.n, host.ctypes.data, dptr.data_ptr(), clusters,
          int(ds.max_len), mid, int(gap_open), int(gap_ext), cons.data_ptr(), ld, cons_len.data_ptr(), center.data_ptr(), work.data_ptr(),
          work.numel(), _stream())
    return cons[:clusters], cons_len[:clusters], center[:clusters]


def consensus_center_sums(length, matches, cluster_ptr, pair_begin=0, sums=None):
    """One block of phase 1 (da_dev_consensus_center_sums): length / matches are int32 device tensors with the alignment results of the
    ordered in-cluster pairs pair_begin, pair_begin + 1, ... (per cluster i ascending, then j != i ascending); every matches / length
    is added, exactly, to its member's two 64-bit limbs.  sums: the (members, 2) int64 tensor (low, high limb) of an earlier block, or
    None to start from zero.  Returns sums."""
    lib = _capi.load()
    _require_cuda(length, "length")
    _require_cuda(matches, "matches")
    if length.dtype != torch.int32 or matches.dtype != torch.int32 or length.numel() != matches.numel():
        raise ValueError("length and matches must be int32 tensors of the same length")
    host, dptr = _cluster_table(cluster_ptr, length.device)
    clusters = len(host) - 1
    if sums is None:
        sums = torch.zeros((max(int(host[-1]), 1), 2), dtype=torch.int64, device=length.device)
    scratch = torch.empty(clusters + 1, dtype=torch.int64, device=length.device)
    length, matches = length.contiguous(), matches.contiguous()
    _call(lib.da_dev_consensus_center_sums, length.data_ptr(), matches.data_ptr(), int(pair_begin), length.numel(), host.ctypes.data,
          dptr.data_ptr(), clusters, scratch.data_ptr(), sums.data_ptr(), _stream())
    return sums


def consensus_pick(sums, cluster_ptr):
    """The centers (da_dev_consensus_pick): per cluster the pooled index of the member whose sum, rounded to a double as math.fsum
    rounds, is largest; the lowest index among equals.  Returns an int32 tensor."""
    lib = _capi.load()
    _require_cuda(sums, "sums")
    host, dptr = _cluster_table(cluster_ptr, sums.device)
    clusters = len(host) - 1
    center = torch.zeros(max(clusters, 1), dtype=torch.int32, device=sums.device)
    _call(lib.da_dev_consensus_pick, sums.data_ptr(), dptr.data_ptr(), clusters, center.data_ptr(), _stream())
    return center[:clusters]


def consensus_vote(ds, cluster_ptr, center, ops, length=None):
    """The column vote (da_dev_consensus_vote) of every cluster on given ops rows: center an int32 device tensor of pooled indices,
    ops a (rows, ld_ops) uint8 tensor holding, cluster after cluster, the paths of the center as sequence1 with every other member in
    ascending order ('D' / 'U' / 'L', 0 past a row's end), length their int32 lengths or None.  Returns ``(cons, cons_len)``."""
    lib = _capi.load()
    if ds.codes is None:
        raise ValueError("call nw_encode first")
    dev = ds.residues.device
    host, dptr = _cluster_table(cluster_ptr, dev)
    clusters = len(host) - 1
    rows = int(host[-1]) - clusters
    _require_cuda(ops, "ops")
    if ops.dtype != torch.uint8 or ops.dim() != 2 or ops.shape[0] < rows:
        raise ValueError("ops must be a (rows, ld_ops) uint8 tensor with a row per member other than the center")
    ops = ops.contiguous()
    ld = max(int(ds.max_len), 1)
    cons = torch.zeros((max(clusters, 1), ld), dtype=torch.uint8, device=dev)
    cons_len = torch.zeros(max(clusters, 1), dtype=torch.int32, device=dev)
    carry = torch.empty(25 * ld, dtype=torch.int32, device=dev)
    center = center.contiguous()
    length = None if length is None else length.contiguous()
    _call(lib.da_dev_consensus_vote, ds.codes.data_ptr(), ds.offsets.data_ptr(), dptr.data_ptr(), center.data_ptr(), 0, clusters, ops.data_ptr(),
          ops.shape[1], None if length is None else length.data_ptr(), 0, rows, carry.data_ptr(), cons.data_ptr(), ld,
          cons_len.data_ptr(), int(ds.max_len), _stream())
    return cons[:clusters], cons_len[:clusters]


def symmetrize(mat, n, kind=DA_OUT_F64):
    _call(_capi.load().da_dev_symmetrize, mat.data_ptr(), n, mat.stride(0), kind, _stream())
    return mat


def widen(compact, is_nw, n_hash=0, out=None):
    """uint16 block (int16 tensor) -> float64 with the reference's divide."""
    if out is None:
        out = torch.empty(compact.shape, dtype=torch.float64, device=compact.device)
    assert compact.is_contiguous() and out.is_contiguous()
    _call(_capi.load().da_dev_widen, compact.data_ptr(), out.data_ptr(), compact.numel(), 1 if is_nw else 0,
                                          int(n_hash), _stream())
    return out


def upper_histogram(compact, n, nbins):
    """uint64 histogram (int64 tensor) of the strict upper triangle of an n x n uint16 count matrix."""
    hist = torch.zeros(nbins, dtype=torch.int64, device=compact.device)
    _call(_capi.load().da_dev_upper_histogram, compact.data_ptr(), compact.stride(0), n, int(nbins),
                                                    hist.data_ptr(), _stream())
    return hist


def extract_edges(compact, n, keep, capacity, include_diagonal=True):
    """Append (i, j, value) of the upper-triangle entries whose value v has keep[v] != 0.
    Returns (i, j, v, count): int32, int32, int16 tensors of `capacity` slots and the int64 count tensor."""
    return _extract_edges(_capi.load().da_dev_extract_edges, compact, (n,), keep, capacity, include_diagonal)


def _extract_edges(entry, mat, shape, keep, capacity, include_diagonal):
    """extract_edges / extract_edges_rows: `shape` is what the entry point takes between the matrix's row stride and the keep table"""
    dev = mat.device
    keep_t = torch.as_tensor(np.ascontiguousarray(keep, np.uint8)).to(dev)
    ei, ej, ev = _edge_slots(capacity, dev, (torch.int32, torch.int32, torch.int16))
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    _call(entry, mat.data_ptr(), mat.stride(0), *shape, keep_t.data_ptr(), keep_t.numel(), 1 if include_diagonal else 0, ei.data_ptr(),
          ej.data_ptr(), ev.data_ptr(), int(capacity), cnt.data_ptr(), _stream())
    return ei, ej, ev, cnt


def unique_table(planes, unique, n_hash):
    """symmetric uint16 count table of the plan's unique strings (K2 on `unique` rows) with 16-byte aligned rows -- what
    unique_rows / expand_unique read in 16-byte units"""
    ld = -(-int(unique) // 8) * 8
    buf = torch.empty((int(unique), ld), dtype=torch.int16, device=planes.device)
    return mh_compare(planes, int(unique), n_hash, 0, int(unique), True, DA_OUT_COMPACT, out=buf)


def unique_rows(table, plan, out=None):
    """the n x n uint16 matrix without its duplicate rows (da_dev_unique_rows): [unique][ceil8(n)] int16; row i of the full matrix
    = row uidx[i] of it for the columns j >= i"""
    lib = _capi.load()
    ld = -(-plan.n // 8) * 8
    if out is None:
        out = torch.empty((plan.unique, ld), dtype=torch.int16, device=table.device)
    _call(lib.da_dev_unique_rows, table.data_ptr(), table.stride(0), plan.ptr(), out.data_ptr(), _stream())
    return out


def upper_histogram_rows(rows, plan, nbins):
    """upper_histogram of the full matrix read through the plan's row map"""
    hist = torch.zeros(nbins, dtype=torch.int64, device=rows.device)
    _call(_capi.load().da_dev_upper_histogram_rows, rows.data_ptr(), rows.stride(0), plan.c.d_uidx, plan.n, int(nbins),
                                                         hist.data_ptr(), _stream())
    return hist


def extract_edges_rows(rows, plan, keep, capacity, include_diagonal=True):
    """extract_edges of the full matrix read through the plan's row map"""
    return _extract_edges(_capi.load().da_dev_extract_edges_rows, rows, (plan.c.d_uidx, plan.n), keep, capacity, include_diagonal)


def edges_to_csr(ei, ej, ev, n_edges, n):
    """(i <= j, code) device edge list -> symmetric CSR on the device (da_dev_edges_to_csr): returns (ptr int64[n+1], adj int32[nnz],
    codes int16[nnz] (uint16 bit pattern), loops int16[n] (0xFFFF = no self-loop)) as device tensors; nnz = ptr[n]"""
    lib = _capi.load()
    dev = ei.device
    m, n = int(n_edges), int(n)
    nbytes = int(lib.da_dev_edges_to_csr_bytes(m, n))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
    adj = torch.empty(max(2 * m, 1), dtype=torch.int32, device=dev)
    codes = torch.empty(max(2 * m, 1), dtype=torch.int16, device=dev)
    loops = torch.empty(max(n, 1), dtype=torch.int16, device=dev)
    _call(lib.da_dev_edges_to_csr, ei.data_ptr(), ej.data_ptr(), ev.data_ptr(), m, n, work.data_ptr(), nbytes, ptr.data_ptr(),
                                        adj.data_ptr(), codes.data_ptr(), loops.data_ptr(), _stream())
    nnz = int(ptr[n].item())
    return ptr, adj[:nnz], codes[:nnz], loops[:n]


# the degree bins of the decide kernels (csrc/louvain_kernels.hip): a wave per row up to LOUVAIN_WAVE_MAX entries, a workgroup and an LDS
# table up to LOUVAIN_LDS_MAX, a table in the workspace beyond; on a level of at most LOUVAIN_DIRECT_MAX vertices the LDS table is indexed
# by the community id and takes rows of any length.  A row above LOUVAIN_LDS_MAX tries the LDS table (LOUVAIN_LDS_SLOTS slots) first and takes
# the workspace table when its neighbouring communities do not fit
LOUVAIN_WAVE_MAX, LOUVAIN_LDS_MAX, LOUVAIN_DIRECT_MAX, LOUVAIN_LDS_SLOTS = 64, 3072, 4096, 4096


def louvain_workspace_bytes(n, nnz):
    return int(_capi.load().da_dev_louvain_workspace_bytes(int(n), int(nnz)))


def louvain_csr(ptr, adj, codes, loops, values, resolution=1.05, seed=0, weights=True, work=None):
    """The synchronous Louvain (clusterbreak.louvain_sync_dense, reproduced bit for bit) on a canonical symmetric CSR that lies in HBM
    (da_dev_louvain_csr): the tensors `edges_to_csr` returns -- ptr int64[n + 1], adj int32[nnz], codes int16[nnz] (uint16 bit pattern),
    loops int16[n] (0xFFFF = no self-loop; None = none) -- and the host array `values` (weight of entry e = values[codes[e]]).
    weights=False gives every code the weight 1.0.  Returns (membership int32 numpy, ids from 1 in order of first appearance; Q; levels;
    iterations per level).  The call synchronises the current stream.  A CSR that is not canonical raises DynaAlignError
    (DA_ERR_BAD_ARG); symmetry is not checked."""
    lib = _capi.load()
    _require_cuda(ptr, "ptr")
    n = int(ptr.numel()) - 1
    if n < 0:
        raise _capi.DynaAlignError(_capi.DA_ERR_BAD_ARG, "ptr must hold n + 1 row pointers")
    values = np.ascontiguousarray(values, np.float64)
    if not weights:
        values = np.ones(len(values), np.float64)
    if n == 0:
        return np.zeros(0, np.int32), 0.0, 0, []
    for t, name in ((adj, "adj"), (codes, "codes")):
        _require_cuda(t, name)
    if ptr.dtype != torch.int64 or adj.dtype != torch.int32 or codes.element_size() != 2 or (loops is not None and loops.element_size() != 2):
        raise _capi.DynaAlignError(_capi.DA_ERR_BAD_ARG, "ptr int64, adj int32, codes and loops 16-bit")
    nnz = int(adj.numel())
    if int(codes.numel()) != nnz or (loops is not None and int(loops.numel()) < n):
        raise _capi.DynaAlignError(_capi.DA_ERR_BAD_ARG, "adj, codes and loops disagree with ptr in length")
    if int(ptr[n].item()) != nnz:
        raise _capi.DynaAlignError(_capi.DA_ERR_BAD_ARG, "ptr[n] (%d) is not the number of adjacency entries (%d)" % (int(ptr[n].item()), nnz))
    ptr, adj, codes = ptr.contiguous(), adj.contiguous(), codes.contiguous()
    loops = None if loops is None else loops.contiguous()
    work = _work(work, louvain_workspace_bytes(n, nnz), ptr.device)
    member = torch.empty(n, dtype=torch.int32, device=ptr.device)
    q = ctypes.c_double(0.0)
    levels = ctypes.c_int32(0)
    its = (ctypes.c_int32 * 32)()
    _call(lib.da_dev_louvain_csr, n, ptr.data_ptr(), adj.data_ptr() if nnz else None, codes.data_ptr() if nnz else None,
          None if loops is None else loops.data_ptr(), values.ctypes.data if len(values) else None, len(values), float(resolution),
          int(seed) & 0xFFFFFFFF, work.data_ptr(), int(work.numel()), member.data_ptr(), ctypes.byref(q), ctypes.byref(levels), its, _stream())
    return member.cpu().numpy(), float(q.value), int(levels.value), [int(its[i]) for i in range(int(levels.value))]


def components_workspace_bytes(n):
    return int(_capi.load().da_dev_components_workspace_bytes(int(n)))


def _components_buffers(n, dev, sizes, work, nbytes, what):
    work = _work(work, nbytes, dev, _capi.DynaAlignError(_capi.DA_ERR_BAD_ARG, _WORK_TEXT % what), at_least=nbytes)
    member = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    size_t = torch.empty(max(n, 1), dtype=torch.int32, device=dev) if sizes else None
    return work, member, size_t


def _components_out(n, member, size_t, count):
    c = int(count.value)
    member = member[:n].cpu().numpy()
    return (member, c, size_t[:c].cpu().numpy()) if size_t is not None else (member, c)


def components_edges(ei, ej, n, codes=None, min_code=0, sizes=False, work=None):
    """The connected components (clusterbreak.components_dense, reproduced element for element) of an edge list that lies in HBM
    (da_dev_components_edges): ``ei`` / ``ej`` int32 device tensors of equal length, any order, either orientation, repeats and self-loops
    allowed; ``n`` vertices.  ``codes`` (16-bit device tensor, uint16 bit pattern, one per edge): only the edges with code >= ``min_code``
    count, so one list can be cut at several thresholds.  Returns (membership int32 numpy, ids from 1 in order of first appearance;
    n_components[; sizes int32 numpy, one per component]).  Synchronises the current stream.  An endpoint outside [0, n) -- of a filtered
    edge too -- raises DynaAlignError (DA_ERR_BAD_ARG)."""
    lib = _capi.load()
    n = int(n)
    if n < 0:
        raise _capi.DynaAlignError(_capi.DA_ERR_BAD_ARG, "n must not be negative")
    for t, name in ((ei, "ei"), (ej, "ej")) + (((codes, "codes"),) if codes is not None else ()):
        _require_cuda(t, name)
    if ei.dtype != torch.int32 or ej.dtype != torch.int32 or (codes is not None and codes.element_size() != 2):
        raise _capi.DynaAlignError(_capi.DA_ERR_BAD_ARG, "ei and ej int32, codes 16-bit")
    m = int(ei.numel())
    if int(ej.numel()) != m or (codes is not None and int(codes.numel()) != m):
        raise _capi.DynaAlignError(_capi.DA_ERR_BAD_ARG, "ei, ej and codes differ in length")
    if not 0 <= int(min_code) <= 65536:
        raise _capi.DynaAlignError(_capi.DA_ERR_BAD_ARG, "min_code must be in 0 .. 65536")
    if n == 0:
        return (np.zeros(0, np.int32), 0, np.zeros(0, np.int32)) if sizes else (np.zeros(0, np.int32), 0)
    ei, ej = ei.contiguous(), ej.contiguous()
    codes = None if codes is None else codes.contiguous()
    work, member, size_t = _components_buffers(n, ei.device, sizes, work, components_workspace_bytes(n), "components_workspace_bytes(n)")
    count = ctypes.c_int64(0)
    _call(lib.da_dev_components_edges, ei.data_ptr() if m else None, ej.data_ptr() if m else None, None if codes is None or not m else codes.data_ptr(),
          int(min_code), m, n, work.data_ptr(), int(work.numel()), member.data_ptr(), None if size_t is None else size_t.data_ptr(),
          ctypes.byref(count), _stream())
    return _components_out(n, member, size_t, count)


def components_csr(ptr, adj, symmetric=True, sizes=False, work=None):
    """The connected components of a CSR that lies in HBM (da_dev_components_csr): ``ptr`` int64[n + 1] and ``adj`` int32[ptr[n]], exactly
    what `edges_to_csr` and the kNN graphs of MinHashSession return (codes and loops are not needed).  ``symmetric=True`` says both
    directions of every edge are present: only the entries with adj > row are united, half the work; pass False for any other CSR.
    Returns (membership int32 numpy, n_components[, sizes]).  Synchronises the current stream.  Row pointers that do not start at 0,
    decrease or leave [0, nnz], and a neighbour outside [0, n), raise DynaAlignError (DA_ERR_BAD_ARG)."""
    lib = _capi.load()
    _require_cuda(ptr, "ptr")
    n = int(ptr.numel()) - 1
    if n < 0:
        raise _capi.DynaAlignError(_capi.DA_ERR_BAD_ARG, "ptr must hold n + 1 row pointers")
    if n == 0:
        return (np.zeros(0, np.int32), 0, np.zeros(0, np.int32)) if sizes else (np.zeros(0, np.int32), 0)
    _require_cuda(adj, "adj")
    if ptr.dtype != torch.int64 or adj.dtype != torch.int32:
        raise _capi.DynaAlignError(_capi.DA_ERR_BAD_ARG, "ptr int64, adj int32")
    nnz = int(adj.numel())
    if int(ptr[n].item()) != nnz:
        raise _capi.DynaAlignError(_capi.DA_ERR_BAD_ARG, "ptr[n] (%d) is not the number of adjacency entries (%d)" % (int(ptr[n].item()), nnz))
    ptr, adj = ptr.contiguous(), adj.contiguous()
    work, member, size_t = _components_buffers(n, ptr.device, sizes, work, components_workspace_bytes(n), "components_workspace_bytes(n)")
    count = ctypes.c_int64(0)
    _call(lib.da_dev_components_csr, n, ptr.data_ptr(), adj.data_ptr() if nnz else None, 1 if symmetric else 0, work.data_ptr(), int(work.numel()),
          member.data_ptr(), None if size_t is None else size_t.data_ptr(), ctypes.byref(count), _stream())
    return _components_out(n, member, size_t, count)


def similarity_mh(ds, k, n_hash, seeds, out=None):
    """similarityMH (src/minHash.cpp:119-188) on a device-resident set, one C call: K1 + K1b + K2, with byte-identical
    sequences collapsed first when that pays (da_dev_similarity_mh).  Returns the (n, n) float64 tensor."""
    lib = _capi.load()
    seeds = _seeds_tensor(seeds, ds.residues.device)
    _require_cuda(ds.residues, "residues")
    n = ds.n
    if out is None:
        out = torch.empty((max(n, 1), max(n, 1)), dtype=torch.float64, device=ds.residues.device)
    _call(lib.da_dev_similarity_mh, ds.residues.data_ptr(), ds.offsets.data_ptr(), n, ds.total, int(k), int(n_hash),
                                         seeds.data_ptr(), out.data_ptr(), out.stride(0), _stream())
    return out


def similarity_mh_cross(dx, dy, k, n_hash, seeds, out=None):
    """similarityMH_cross on two device-resident sets, one C call (da_dev_similarity_mh_cross): K1 per side, K1b on the union,
    the rectangle compare -- or, when collapsing byte-identical strings per side pays, the table of the unique strings and
    its rectangular row expansion.  Returns the (m, n) float64 tensor."""
    lib = _capi.load()
    seeds = _seeds_tensor(seeds, dx.residues.device)
    _require_cuda(dx.residues, "residues of x")
    _require_cuda(dy.residues, "residues of y")
    if out is None:
        out = _alloc_out(dx.n, dy.n, DA_OUT_F64, dx.residues.device, None)
    _call(lib.da_dev_similarity_mh_cross, dx.residues.data_ptr(), dx.offsets.data_ptr(), dx.n, dx.total, dy.residues.data_ptr(),
                                               dy.offsets.data_ptr(), dy.n, dy.total, int(k), int(n_hash), seeds.data_ptr(),
                                               out.data_ptr(), out.stride(0), _stream())
    return out


def _block(keys, dtype, n=None):
    """(rows, n, ld) of a block of keys: a tensor of `dtype` (or of one of a tuple) of shape (rows, >= n), any row stride and base address,
    whose first n columns (all of them by default) are the block"""
    _require_cuda(keys, "keys")
    assert keys.dim() == 2 and keys.dtype in (dtype if isinstance(dtype, tuple) else (dtype,)) and (keys.shape[1] <= 1 or keys.stride(1) == 1)
    rows, n = int(keys.shape[0]), int(keys.shape[1] if n is None else n)
    assert 0 <= n <= keys.shape[1]
    return rows, n, (int(keys.stride(0)) if rows > 1 else max(n, 1))


def _rank_table(rank):
    """the 65536-entry table of uint16 ranks of topk_rows and upper_extrema"""
    _require_cuda(rank, "rank table")
    assert rank.dtype == torch.int16 and rank.numel() == 65536 and rank.is_contiguous()
    return rank.data_ptr()


def _topk(entry, entry_self, keys, block, order, top, self_col0, want_self):
    """topk_rows / topk_ranks: `block` = (rows, n, ld) of the keys, `order` what the entry points take between ld and top.  A block without
    rows is not handed to the library (its address is NULL)."""
    rows = block[0]
    idx, key = _topk_out(rows, top, keys.dtype, keys.device)
    out = (idx.data_ptr(), key.data_ptr(), idx.shape[1])
    if self_col0 is None:
        if want_self:
            raise ValueError("want_self needs self_col0")
        if rows > 0:
            _call(entry, keys.data_ptr(), *block, *order, int(top), *out, _stream())
        return idx[:rows], key[:rows]
    own = torch.zeros(max(rows, 1), dtype=keys.dtype, device=keys.device) if want_self else None
    if rows > 0:
        _call(entry_self, keys.data_ptr(), *block, *order, int(top), int(self_col0), *out, None if own is None else own.data_ptr(), _stream())
    return (idx[:rows], key[:rows], own[:rows]) if want_self else (idx[:rows], key[:rows])


def topk_rows(keys, top, rank=None, rank_bits=0, self_col0=None, want_self=False):
    """Exact top-k per row of a block of uint16 keys (an int16 tensor of shape (rows, n), any row stride and base address), by
    (rank descending, column ascending): rank = rank[key] (a 65536-entry int16 tensor of uint16 ranks, all below 2 ** rank_bits) or
    the key itself (da_dev_topk_rows).  Returns (idx int32 (rows, top), key int16 (rows, top)): numpy's
    argsort(-rank_of_row, kind="stable")[:top] and the keys found there.
    self_col0: the block is rows [self_col0, self_col0 + rows) of a square problem and row r's own column self_col0 + r is left out of
    its selection (da_dev_topk_rows_self; 1 <= top <= n - 1); with want_self a third result, int16 (rows,), holds the key found at the
    own column (rows whose own column is outside [0, n) keep 0)."""
    lib = _capi.load()
    block = _block(keys, torch.int16)
    order = (None if rank is None else _rank_table(rank), int(rank_bits))
    return _topk(lib.da_dev_topk_rows, lib.da_dev_topk_rows_self, keys, block, order, top, self_col0, want_self)


def topk_ranks(keys, top, nbins, self_col0=None, want_self=False):
    """Exact top-k per row of a block of uint32 value ranks (an int32 tensor of shape (rows, n) holding the uint32 bit patterns, any row
    stride and base address; every key < nbins), by (rank descending, column ascending) (da_dev_topk_ranks).  Returns (idx int32
    (rows, top), key int32 (rows, top)): numpy's argsort(-row, kind="stable")[:top] and the ranks found there.  nbins only places the
    digits of the radix select.  self_col0 / want_self as in topk_rows (da_dev_topk_ranks_self; 1 <= top <= n - 1): the third result,
    int32 (rows,), holds the rank found at the own column (rows whose own column is outside [0, n) keep 0)."""
    lib = _capi.load()
    return _topk(lib.da_dev_topk_ranks, lib.da_dev_topk_ranks_self, keys, _block(keys, torch.int32), (int(nbins),), top, self_col0, want_self)


def similarity_mh_knn(ds, k, n_hash, seeds, top):
    """The nearest-neighbour lists of a device-resident set, one C call (da_dev_similarity_mh_knn): (idx int32 (n, top), val float64
    (n, top)).  Row i lists the `top` columns j != i of row i of similarity_mh(ds, ...) by value descending, then column ascending; the
    n x n matrix never exists.  top is NOT clamped here (1 <= top <= n - 1)."""
    lib = _capi.load()
    seeds = _seeds_tensor(seeds, ds.residues.device)
    _require_cuda(ds.residues, "residues")
    idx, val = _topk_out(ds.n, top, torch.float64, ds.residues.device)
    _call(lib.da_dev_similarity_mh_knn, ds.residues.data_ptr(), ds.offsets.data_ptr(), ds.n, int(k), int(n_hash), seeds.data_ptr(), int(top),
                                             idx.data_ptr(), val.data_ptr(), idx.shape[1], _stream())
    return idx[:ds.n], val[:ds.n]


def knn_edges(idx, key, mode="union", is_nw=False, self_key=None, self_code=0, loops=True):
    """Nearest-neighbour lists -> the (i <= j, code) edge list of their kNN graph on the device (da_dev_knn_edges).  idx int32 (n, top) and
    key int16 (n, top) (uint16 bit pattern) as topk_rows with self_col0 returns them; an entry is live when its key stands for a value > 0
    (key != 0, or key >> 8 != 0 with is_nw).  mode "union" keeps {i, j} when j is in i's list or i in j's, "mutual" when both.  loops: every
    vertex also gets (r, r, self_key[r]), or (r, r, self_code) without self_key.  Returns (ei int32, ej int32, ev int16, n_edges) with
    ei <= ej, grouped by emitting row (NOT sorted by (i, j)): what edges_to_csr takes."""
    lib = _capi.load()
    _require_cuda(idx, "idx")
    _require_cuda(key, "key")
    if mode not in ("union", "mutual"):
        raise ValueError("mode must be 'union' or 'mutual'")
    assert idx.dim() == 2 and idx.dtype == torch.int32 and key.dtype == torch.int16 and key.shape == idx.shape
    idx, key = idx.contiguous(), key.contiguous()
    n, top = int(idx.shape[0]), int(idx.shape[1])
    dev = idx.device
    if self_key is not None:
        _require_cuda(self_key, "self_key")
        self_key = self_key.contiguous()
        assert self_key.dtype == torch.int16 and self_key.numel() == n
    cap = n * (top + (1 if loops else 0))
    nbytes = int(lib.da_dev_knn_edges_bytes(n, top))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ei, ej, ev = _edge_slots(cap, dev, (torch.int32, torch.int32, torch.int16))
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    _call(lib.da_dev_knn_edges, idx.data_ptr(), key.data_ptr(), top, n, top, _capi.DA_KNN_MUTUAL if mode == "mutual" else _capi.DA_KNN_UNION,
                                     1 if is_nw else 0, None if self_key is None else self_key.data_ptr(), int(self_code), 1 if loops else 0,
                                     work.data_ptr(), nbytes, ei.data_ptr(), ej.data_ptr(), ev.data_ptr(), count.data_ptr(), _stream())
    m = int(count.item())
    return ei[:m], ej[:m], ev[:m], m


def similarity_mh_cross_topk(dx, dy, k, n_hash, seeds, top):
    """similarityMH_cross followed by the per-row top-k selection on two device-resident sets, one C call
    (da_dev_similarity_mh_cross_topk): (idx int32 (m, top), val float64 (m, top)).  Row i lists the `top` columns of
    row i of similarity_mh_cross(dx, dy, ...) by value descending, then column ascending; the m x n matrix never exists --
    row blocks of uint16 counts are selected from as they are computed.  top is NOT clamped here (1 <= top <= n)."""
    lib = _capi.load()
    seeds = _seeds_tensor(seeds, dx.residues.device)
    _require_cuda(dx.residues, "residues of x")
    _require_cuda(dy.residues, "residues of y")
    idx, val = _topk_out(dx.n, top, torch.float64, dx.residues.device)
    _call(lib.da_dev_similarity_mh_cross_topk, dx.residues.data_ptr(), dx.offsets.data_ptr(), dx.n, dy.residues.data_ptr(),
                                                    dy.offsets.data_ptr(), dy.n, int(k), int(n_hash), seeds.data_ptr(), int(top),
                                                    idx.data_ptr(), val.data_ptr(), idx.shape[1], _stream())
    return idx[:dx.n], val[:dx.n]


def rect_histogram(keys, nbins):
    """uint64 histogram (int64 tensor of nbins entries) of a whole block of uint16 keys; keys >= nbins are ignored (da_dev_rect_histogram)"""
    rows, n, ld = _block(keys, torch.int16)
    hist = torch.zeros(int(nbins), dtype=torch.int64, device=keys.device)
    _call(_capi.load().da_dev_rect_histogram, keys.data_ptr(), rows, n, ld, int(nbins), hist.data_ptr(), _stream())
    return hist


def threshold_rows(keys, keep, capacity=None):
    """The flagged entries of a block of uint16 keys as CSR: (rowptr int64 (rows + 1), j int32, key int16 (uint16 bit pattern)) -- per row
    the columns whose key v has keep[v] != 0 (keys >= len(keep) are never kept), ascending, row r at rowptr[r] : rowptr[r + 1]
    (da_dev_threshold_rows_count, then da_dev_threshold_rows_emit).  capacity=None sizes j / key from the count (one 8-byte read-back);
    otherwise they hold `capacity` slots and entries beyond it are counted in rowptr but not stored."""
    lib = _capi.load()
    block = _block(keys, torch.int16)
    keep_t = keep if torch.is_tensor(keep) else torch.as_tensor(np.ascontiguousarray(keep, np.uint8))
    keep_t = keep_t.to(keys.device).contiguous()
    assert keep_t.dtype == torch.uint8
    return _threshold(lib.da_dev_threshold_rows_count, lib.da_dev_threshold_rows_emit, keys, block, (keep_t.data_ptr(), keep_t.numel()), capacity)


def _threshold(entry_count, entry_emit, keys, block, mask, capacity):
    """threshold_rows / threshold_ranks: the count call, the read-back of rowptr[rows] unless a capacity is given, the emit call.  `block` =
    (rows, n, ld) of the keys, `mask` what the two entry points take between ld and rowptr: what says which entries are kept."""
    rows, dev = block[0], keys.device
    rowptr = torch.zeros(rows + 1, dtype=torch.int64, device=dev)
    if rows > 0:
        nbytes = int(_capi.load().da_dev_threshold_rows_workspace_bytes(rows))
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _call(entry_count, keys.data_ptr(), *block, *mask, rowptr.data_ptr(), work.data_ptr(), nbytes, _stream())
    cap = int(rowptr[rows].item()) if capacity is None else int(capacity)
    j, key = _edge_slots(cap, dev, (torch.int32, keys.dtype))
    if rows > 0 and cap > 0:
        _call(entry_emit, keys.data_ptr(), *block, *mask, rowptr.data_ptr(), j.data_ptr(), key.data_ptr(), cap, _stream())
    return rowptr, j[:cap], key[:cap]


def nw_codes_to_ranks(codes, rank, max_len, out=None):
    """The value ranks of a block of PACK32 codes (matches << 16 | length; an int32 tensor (rows, n)) through ``rank``, the table of
    ``nw_value_ranks(max_len)`` as a flat int32 tensor on the device: a code outside the table's domain gets rank 0
    (da_dev_nw_codes_to_ranks).  ``out=None`` returns a new tensor, ``out=codes`` converts in place."""
    rows, n, ld = _block(codes, torch.int32)
    _require_cuda(rank, "rank table")
    ml = int(max_len)
    assert rank.dtype == torch.int32 and rank.is_contiguous() and rank.numel() == (2 * ml + 1) * (ml + 1)
    if out is None:
        out = torch.empty((rows, n), dtype=torch.int32, device=codes.device)
    orows, on, old = _block(out, torch.int32)
    assert (orows, on) == (rows, n)
    _call(_capi.load().da_dev_nw_codes_to_ranks, codes.data_ptr(), rows, n, ld, ml, rank.data_ptr(), out.data_ptr(), old, _stream())
    return out


def rank_histogram(keys, nbins, triangle=False, row_begin=0, col_begin=0):
    """uint64 histogram (int64 tensor of nbins entries) of a block of uint32 keys; keys >= nbins are ignored (da_dev_rank_histogram).
    triangle: the block is rows row_begin ... x columns col_begin ... of a square problem and only global column > global row counts."""
    rows, n, ld = _block(keys, torch.int32)
    hist = torch.zeros(int(nbins), dtype=torch.int64, device=keys.device)
    _call(_capi.load().da_dev_rank_histogram, keys.data_ptr(), rows, n, ld, int(nbins), hist.data_ptr(), int(bool(triangle)), int(row_begin),
          int(col_begin), _stream())
    return hist


def threshold_ranks(keys, r_min, nbins, triangle=False, row_begin=0, col_begin=0, capacity=None):
    """The entries of a block of uint32 keys with r_min <= key < nbins as CSR: (rowptr int64 (rows + 1), j int32, key int32 (uint32 bit
    pattern)) -- per row the kept columns (local to the block), ascending (da_dev_threshold_ranks_count, then da_dev_threshold_ranks_emit).
    triangle: only global column >= global row, the diagonal included.  capacity as in ``threshold_rows``."""
    lib = _capi.load()
    mask = (int(r_min), int(nbins), int(bool(triangle)), int(row_begin), int(col_begin))
    return _threshold(lib.da_dev_threshold_ranks_count, lib.da_dev_threshold_ranks_emit, keys, _block(keys, torch.int32), mask, capacity)


def upper_extrema(keys, n, rank=None, row_begin=0, col_begin=0):
    """Per row of a block of keys -- rows row_begin ... x columns col_begin ... col_begin + n of a square problem, held in the first n columns
    of an int16 (uint16 keys) or int32 (uint32 value ranks) tensor with any row stride and base address -- the extremes of the elements whose
    global column is greater than the global row: an int32 tensor (rows, 5) of {min, first local column of the min, max, first local column
    of the max, diagonal element} (struct da_row_extrema; the ranks are uint32 bit patterns, a column is -1 where the row has no such
    element, the diagonal 0xFFFFFFFF where it lies outside the block).  rank: the 65536-entry int16 table of ``nw_code_ranks`` on the device,
    uint16 keys only -- the comparison is then on rank[key] and the record holds ranks (da_dev_upper_extrema / da_dev_upper_extrema32)."""
    lib = _capi.load()
    rows, n, ld = _block(keys, (torch.int16, torch.int32), n)
    rec = torch.empty((max(rows, 1), _capi.ROW_EXTREMA_WORDS), dtype=torch.int32, device=keys.device)
    if keys.dtype == torch.int16:
        _call(lib.da_dev_upper_extrema, keys.data_ptr(), rows, n, ld, None if rank is None else _rank_table(rank), int(row_begin), int(col_begin),
              rec.data_ptr(), _stream())
    else:
        assert rank is None, "uint32 keys are value ranks already"
        _call(lib.da_dev_upper_extrema32, keys.data_ptr(), rows, n, ld, int(row_begin), int(col_begin), rec.data_ptr(), _stream())
    return rec[:rows]


def similarity_mh_cross_edges(dx, dy, k, n_hash, seeds, thresh_p=None, threshold=None, capacity=None):
    """The threshold form of similarity_mh_cross on two device-resident sets, one C call (da_dev_similarity_mh_cross_edges):
    (threshold, rowptr int64 (m + 1), j int32, w float64) -- CSR over the rows of x of the entries with R >= threshold and R > 0, columns
    ascending, w bit for bit R.  threshold is not None: the absolute form; otherwise the type-7 quantile thresh_p (default 0.8) of all
    m * n entries.  With a capacity, j / w hold that many slots and rowptr is complete even when rowptr[m] exceeds it; capacity=None
    starts from a guess and calls again when the result does not fit."""
    lib = _capi.load()
    seeds = _seeds_tensor(seeds, dx.residues.device)
    _require_cuda(dx.residues, "residues of x")
    _require_cuda(dy.residues, "residues of y")
    dev = dx.residues.device
    thresh, is_q = (float(threshold), 0) if threshold is not None else (0.8 if thresh_p is None else float(thresh_p), 1)
    rowptr = torch.empty(max(dx.n, 0) + 1, dtype=torch.int64, device=dev)
    thr, cnt = ctypes.c_double(0.0), ctypes.c_int64(0)
    cap = max(4 * max(dx.n, 0), 1 << 20) if capacity is None else int(capacity)
    while True:
        j, w = _edge_slots(cap, dev, (torch.int32, torch.float64))
        _call(lib.da_dev_similarity_mh_cross_edges, dx.residues.data_ptr(), dx.offsets.data_ptr(), dx.n, dy.residues.data_ptr(),
                                                         dy.offsets.data_ptr(), dy.n, int(k), int(n_hash), seeds.data_ptr(), thresh, is_q,
                                                         rowptr.data_ptr(), j.data_ptr(), w.data_ptr(), cap, ctypes.addressof(thr),
                                                         ctypes.addressof(cnt), _stream())
        if capacity is not None or cnt.value <= cap:
            break
        cap = cnt.value
    stored = min(cnt.value, max(cap, 0))
    return thr.value, rowptr, j[:stored], w[:stored]


def _sig_block(sig, n_hash):
    _require_cuda(sig, "signatures")
    if sig.dim() != 2 or sig.element_size() != 4 or sig.stride(1) != 1 or sig.shape[1] < int(n_hash):
        raise ValueError("signatures must be a 2-d tensor of 32-bit words with unit column stride and at least n_hash columns")
    return sig.shape[0], sig.stride(0)


def lsh_workspace_bytes(n, bands):
    return int(_capi.load().da_dev_lsh_workspace_bytes(int(n), int(bands)))


def _lsh_work(work, n, bands, device):
    return _work(work, lambda: lsh_workspace_bytes(n, bands), device, ValueError(_WORK_TEXT % "lsh_workspace_bytes(n, bands)"))


def _listed_triples(i, j, band, device):
    """-> (i, j, band as int32 device tensors, their number m, the zeroed count int16 and keep uint8 results) of the verify calls"""
    ti, tj, tb = ((a if torch.is_tensor(a) else torch.as_tensor(np.ascontiguousarray(a, np.int32))).to(device=device, dtype=torch.int32).contiguous()
                  for a in (i, j, band))
    if not ti.numel() == tj.numel() == tb.numel():
        raise ValueError("i, j and band must have the same number of entries")
    m = int(ti.numel())
    return ti, tj, tb, m, torch.zeros(max(m, 1), dtype=torch.int16, device=device), torch.zeros(max(m, 1), dtype=torch.uint8, device=device)


def lsh_band_keys(sig, n_hash, bands, rows):
    """The bucket keys of LSH banding (da_dev_lsh_band_keys): ``sig`` (n, >= n_hash) 32-bit -> (keys int64 (n, bands), ids int32 (n, bands)):
    keys[i, t] = t << 48 | 48 bits of a hash of sig[i, t * rows:(t + 1) * rows], ids[i, t] = i.  Reads columns < bands * rows only."""
    lib = _capi.load()
    n, ld = _sig_block(sig, n_hash)
    keys = torch.empty((n, max(int(bands), 1)), dtype=torch.int64, device=sig.device)
    ids = torch.empty((n, max(int(bands), 1)), dtype=torch.int32, device=sig.device)
    _call(lib.da_dev_lsh_band_keys, sig.data_ptr(), n, ld, int(n_hash), int(bands), int(rows), keys.data_ptr(), ids.data_ptr(), _stream())
    return keys, ids


def lsh_verify_pairs(sig, n_hash, bands, rows, threshold, i, j, band):
    """The per-pair decision of the LSH pipeline on listed triples (da_dev_lsh_verify_pairs) -> (count int16-as-uint16 tensor, keep uint8):
    count = equal columns of rows i and j; keep = 1 when ``band`` agrees in all its columns, no earlier band does and
    count / n_hash >= threshold."""
    lib = _capi.load()
    n, ld = _sig_block(sig, n_hash)
    ti, tj, tb, m, count, keep = _listed_triples(i, j, band, sig.device)
    _call(lib.da_dev_lsh_verify_pairs, sig.data_ptr(), n, ld, int(n_hash), int(bands), int(rows), float(threshold), ti.data_ptr(), tj.data_ptr(),
          tb.data_ptr(), m, count.data_ptr(), keep.data_ptr(), _stream())
    return count[:m], keep[:m]


def lsh_edges(sig, n_hash, bands, rows, threshold, max_candidates=1 << 32, capacity=None, work=None):
    """The LSH threshold graph of resident signatures (da_dev_lsh_edges) -> (i int32, j int32, count int16-as-uint16), sorted by (i, j),
    diagonal included (count n_hash); weight = count / n_hash.  ``capacity=None``: a first call counts, a second one fills; an int: one
    call, and at most that many edges are returned (``mh_lsh_last_route()["edges"]`` has the full number).  Synchronises the stream."""
    lib = _capi.load()
    n, ld = _sig_block(sig, n_hash)
    work = _lsh_work(work, n, bands, sig.device)
    m = ctypes.c_int64(0)

    def run(cap, ti, tj, tc):
        _call(lib.da_dev_lsh_edges, sig.data_ptr(), n, ld, int(n_hash), int(bands), int(rows), float(threshold), int(max_candidates),
              work.data_ptr(), work.numel(), ti, tj, tc, cap, ctypes.byref(m), _stream())
        return m.value
    return _count_then_fill(run, capacity, sig.device, (torch.int32, torch.int32, torch.int16))


def lsh_components(sig, n_hash, bands, rows, threshold, max_candidates=1 << 32, sizes=False, work=None):
    """The connected components of the LSH threshold graph of resident signatures (da_dev_lsh_components): what
    ``clusterbreak.components_dense`` gives on the edges of `lsh_edges` for the same arguments -- near-duplicate families, single-linkage
    clusters at the cut -- without emitting, sorting or returning an edge: the kept candidate pairs go straight into the union step.
    Returns (membership int32 numpy, n_components[, sizes]).  ``work``: `lsh_workspace_bytes` (n, bands) + `components_workspace_bytes` (n)
    bytes.  ``mh_lsh_last_route()["edges"]`` has the number of edges `lsh_edges` would have returned.  Synchronises the stream."""
    lib = _capi.load()
    n, ld = _sig_block(sig, n_hash)
    if n == 0:
        return (np.zeros(0, np.int32), 0, np.zeros(0, np.int32)) if sizes else (np.zeros(0, np.int32), 0)
    nbytes = lsh_workspace_bytes(n, bands) + components_workspace_bytes(n)
    work, member, size_t = _components_buffers(n, sig.device, sizes, work, nbytes, "lsh_workspace_bytes(n, bands) + components_workspace_bytes(n)")
    count = ctypes.c_int64(0)
    _call(lib.da_dev_lsh_components, sig.data_ptr(), n, ld, int(n_hash), int(bands), int(rows), float(threshold), int(max_candidates),
          work.data_ptr(), int(work.numel()), member.data_ptr(), None if size_t is None else size_t.data_ptr(), ctypes.byref(count), _stream())
    return _components_out(n, member, size_t, count)


# The row classes of the selection (lsh_kernels.hip: LSH_KNN_WAVE_MAX, LSH_KNN_LDS_WORDS): a row of up to LSH_KNN_WAVE_MAX entries is sorted
# by one wave, one of up to LSH_KNN_LDS_WORDS whole in LDS by a workgroup, a longer one goes through the radix select first.
LSH_KNN_WAVE_MAX = 64
LSH_KNN_LDS_WORDS = 2048


def lsh_knn_select(ptr, col, count, top, nnz=None, out=None):
    """The per-row selection of the LSH nearest-neighbour lists on a caller's ragged rows (da_dev_lsh_knn_select): ``ptr`` int64 (n + 1),
    ``col`` int32 (>= 0, distinct within a row, any order) and ``count`` int16 (uint16 bit pattern) device tensors -> (idx int32 (n, top),
    key int16 (n, top)): per row the first ``top`` entries by (count descending, column ascending), then -1 / 0.  ``nnz`` (default
    ``col.numel()``): entries at or behind it are not read, whatever ``ptr`` says.  ``out=(idx, key)``: 2-d tensors with at least ``top``
    columns and unit column stride to write into (columns >= top stay untouched).  Asynchronous on the current stream."""
    lib = _capi.load()
    for t, name in ((ptr, "ptr"), (col, "col"), (count, "count")):
        _require_cuda(t, name)
    assert ptr.dtype == torch.int64 and col.dtype == torch.int32 and count.dtype == torch.int16
    assert ptr.is_contiguous() and col.is_contiguous() and count.is_contiguous() and col.numel() == count.numel()
    n = int(ptr.numel()) - 1
    nnz = int(col.numel()) if nnz is None else int(nnz)
    if not 0 <= nnz <= col.numel():
        raise ValueError("nnz must be in 0 .. col.numel()")
    t = _top(top)
    if out is None:
        idx, key = _topk_out(n, top, torch.int16, ptr.device)
    else:
        idx, key = out
        for o, dt in ((idx, torch.int32), (key, torch.int16)):
            _require_cuda(o, "out")
            assert o.dim() == 2 and o.dtype == dt and o.shape[0] >= n and o.shape[1] >= t and o.stride(1) == 1
    _call(lib.da_dev_lsh_knn_select, ptr.data_ptr(), nnz, col.data_ptr(), count.data_ptr(), n, int(top), idx.data_ptr(), idx.stride(0),
          key.data_ptr(), key.stride(0), _stream())
    return idx[:n, :t], key[:n, :t]


def lsh_knn(sig, n_hash, bands, rows, top, threshold=0.0, max_candidates=1 << 32, work=None):
    """The LSH nearest-neighbour lists of resident signatures (da_dev_lsh_knn) -> (idx int32 (n, top), key int16 (n, top), the counts as
    uint16 bit patterns; padding -1 / 0); value = count / n_hash (``widen``).  ``mh_lsh_last_route()["edges"]`` has the number of real
    entries.  Synchronises the stream."""
    lib = _capi.load()
    n, ld = _sig_block(sig, n_hash)
    work = _lsh_work(work, n, bands, sig.device)
    idx, key = _topk_out(n, top, torch.int16, sig.device)
    _call(lib.da_dev_lsh_knn, sig.data_ptr(), n, ld, int(n_hash), int(bands), int(rows), float(threshold), int(top), int(max_candidates),
          work.data_ptr(), work.numel(), idx.data_ptr(), key.data_ptr(), _stream())
    return idx[:n], key[:n]


def lsh_index_bytes(n, bands):
    return int(_capi.load().da_dev_lsh_index_bytes(int(n), int(bands)))


def lsh_cross_workspace_bytes(m, bands):
    return int(_capi.load().da_dev_lsh_cross_workspace_bytes(int(m), int(bands)))


def _byte_buffer(t, name, what):
    _require_cuda(t, name)
    if t.dtype != torch.uint8 or not t.is_contiguous():
        raise ValueError("%s must be a contiguous uint8 tensor of %s bytes" % (name, what))
    return t


def lsh_index_build(sig_y, n_hash, bands, rows, out=None):
    """The LSH bucket index of a resident set (da_dev_lsh_index_build): ``sig_y`` (n, >= n_hash) 32-bit -> a uint8 tensor of
    lsh_index_bytes(n, bands) bytes holding the sorted band keys, their row ids and the band table (layout: include/dynaalign.h).  It
    depends on nothing but sig_y, bands and rows, and any number of lsh_cross_edges / lsh_cross_topk / lsh_index_probe calls read it.
    ``out``: a buffer to build into.  Synchronises the stream."""
    lib = _capi.load()
    n, ld = _sig_block(sig_y, n_hash)
    if out is None:
        out = torch.empty(lsh_index_bytes(n, bands), dtype=torch.uint8, device=sig_y.device)
    _byte_buffer(out, "out", "lsh_index_bytes(n, bands)")
    _call(lib.da_dev_lsh_index_build, sig_y.data_ptr(), n, ld, int(n_hash), int(bands), int(rows), out.data_ptr(), out.numel(), _stream())
    return out


def lsh_index_arrays(index, n, bands):
    """Views of a built index by the layout of include/dynaalign.h: (meta int32 (8), band_start int32 (bands + 1), keys int64 (n * bands),
    ids int32 (n * bands)); unsigned values as their signed bit patterns."""
    up = lambda b: -(-b // 256) * 256
    total = int(n) * int(bands)
    at = (-index.data_ptr()) % 256
    out = []
    for count, dtype, size in ((8, torch.int32, 4), (int(bands) + 1, torch.int32, 4), (total, torch.int64, 8), (total, torch.int32, 4)):
        out.append(index[at:at + count * size].view(dtype))
        at += up(count * size)
    return tuple(out)


def lsh_index_probe(index, n, sig_x, n_hash, bands, rows):
    """The lookup of a query batch in a built index (da_dev_lsh_index_probe) -> (lo int32 (m, bands), len int32 (m, bands)): the rows of y
    whose band t equals band t of x[i] are ``ids[lo[i, t]:lo[i, t] + len[i, t]]`` (``lsh_index_arrays``), ascending; len = 0 when there is
    none.  The index is only read.  Synchronises the stream."""
    lib = _capi.load()
    m, ld = _sig_block(sig_x, n_hash)
    _byte_buffer(index, "index", "lsh_index_bytes(n, bands)")
    lo = torch.empty((max(m, 1), max(int(bands), 1)), dtype=torch.int32, device=sig_x.device)
    ln = torch.empty_like(lo)
    _call(lib.da_dev_lsh_index_probe, index.data_ptr(), index.numel(), int(n), sig_x.data_ptr(), m, ld, int(n_hash), int(bands), int(rows),
          lo.data_ptr(), ln.data_ptr(), _stream())
    return lo[:m], ln[:m]


def lsh_cross_verify_pairs(sig_x, sig_y, n_hash, bands, rows, threshold, i, j, band):
    """The per-pair decision of the two-set LSH pipeline on listed triples (da_dev_lsh_cross_verify_pairs), row i of sig_x against row j of
    sig_y -> (count int16-as-uint16 tensor, keep uint8): keep = 1 when ``band`` agrees in all its columns, no earlier band does and
    count / n_hash >= threshold."""
    lib = _capi.load()
    m, ld_x = _sig_block(sig_x, n_hash)
    n, ld_y = _sig_block(sig_y, n_hash)
    ti, tj, tb, cnt, count, keep = _listed_triples(i, j, band, sig_x.device)
    _call(lib.da_dev_lsh_cross_verify_pairs, sig_x.data_ptr(), m, ld_x, sig_y.data_ptr(), n, ld_y, int(n_hash), int(bands), int(rows), float(threshold),
          ti.data_ptr(), tj.data_ptr(), tb.data_ptr(), cnt, count.data_ptr(), keep.data_ptr(), _stream())
    return count[:cnt], keep[:cnt]


def _lsh_cross_operands(index, sig_x, sig_y, n_hash, bands, work):
    m, ld_x = _sig_block(sig_x, n_hash)
    n, ld_y = _sig_block(sig_y, n_hash)
    _byte_buffer(index, "index", "lsh_index_bytes(n, bands)")
    work = _work(work, lambda: lsh_cross_workspace_bytes(m, bands), sig_x.device, ValueError(_WORK_TEXT % "lsh_cross_workspace_bytes(m, bands)"))
    return m, ld_x, n, ld_y, work


def lsh_cross_edges(index, sig_x, sig_y, n_hash, bands, rows, threshold, max_candidates=1 << 32, capacity=None, work=None):
    """The two-set LSH edge list of a query batch against an indexed resident set (da_dev_lsh_cross_edges): ``index`` =
    lsh_index_build(sig_y, n_hash, bands, rows) -> (i int32, j int32, count int16-as-uint16), sorted by (i, j); weight = count / n_hash.
    ``capacity=None``: a first call counts, a second one fills; an int: one call, and at most that many edges are returned
    (``mh_lsh_last_route()["edges"]`` has the full number).  Synchronises the stream."""
    lib = _capi.load()
    m, ld_x, n, ld_y, work = _lsh_cross_operands(index, sig_x, sig_y, n_hash, bands, work)
    got = ctypes.c_int64(0)

    def run(cap, ti, tj, tc):
        _call(lib.da_dev_lsh_cross_edges, index.data_ptr(), index.numel(), sig_x.data_ptr(), m, ld_x, sig_y.data_ptr(), n, ld_y, int(n_hash), int(bands),
              int(rows), float(threshold), int(max_candidates), work.data_ptr(), work.numel(), ti, tj, tc, cap, ctypes.byref(got), _stream())
        return got.value
    return _count_then_fill(run, capacity, sig_x.device, (torch.int32, torch.int32, torch.int16))


def lsh_cross_topk(index, sig_x, sig_y, n_hash, bands, rows, top, threshold=0.0, max_candidates=1 << 32, work=None):
    """The two-set LSH nearest-neighbour lists (da_dev_lsh_cross_topk) -> (idx int32 (m, top), key int16 (m, top), the counts as uint16 bit
    patterns; padding -1 / 0); value = count / n_hash (``widen``).  ``top`` is not clamped to the rows of sig_y.  Synchronises the stream."""
    lib = _capi.load()
    m, ld_x, n, ld_y, work = _lsh_cross_operands(index, sig_x, sig_y, n_hash, bands, work)
    idx, key = _topk_out(m, top, torch.int16, sig_x.device)
    _call(lib.da_dev_lsh_cross_topk, index.data_ptr(), index.numel(), sig_x.data_ptr(), m, ld_x, sig_y.data_ptr(), n, ld_y, int(n_hash), int(bands),
          int(rows), float(threshold), int(top), int(max_candidates), work.data_ptr(), work.numel(), idx.data_ptr(), key.data_ptr(), _stream())
    return idx[:m], key[:m]


def mh_lsh_last_route():
    from .similarity import mh_lsh_last_route as route
    return route()


def nw_rescore_workspace_bytes(pairs, max_len=1024, minimal=False):
    return int(_capi.load().da_dev_nw_rescore_workspace_bytes(int(pairs), int(max_len), 1 if minimal else 0))


def nw_rescore_pairs(dx, dy, i, j, matrix_name="BLOSUM62", gap_open=10, gap_ext=4, work=None):
    """NW ``(matches, length)`` of a resident pair list (da_dev_nw_rescore_pairs): pair p aligns dx[i[p]] as sequence1 with dy[j[p]] as
    sequence2; dx.codes / dy.codes must be filled (nw_encode; dx may be dy); i / j: int32 device tensors.  Sequences of 1 .. 1024 residues,
    mixed freely: the split between the lane-per-pair and the wavefront-per-pair kernel happens on the device.  A pair with an index
    outside its set, an empty sequence or one over 1024 residues gets -1 / -1.  -> (matches int32, length int32); the identity is
    matches / length.  work: a uint8 device tensor of at least nw_rescore_workspace_bytes(pairs, minimal=True) bytes, any alignment
    (allocated if None); a smaller one means more launches, never another result.  Synchronises the stream once on the way; the results
    are ordered on the current stream like any other launch.  ``nw_lsh_last_route()`` has the short and long counts."""
    lib = _capi.load()
    if dx.codes is None or dy.codes is None:
        raise ValueError("call nw_encode on both sets first")
    mid = _matrix_id(lib, matrix_name)
    _require_cuda(i, "i")
    _require_cuda(j, "j")
    if i.dtype != torch.int32 or j.dtype != torch.int32 or i.numel() != j.numel():
        raise ValueError("i and j must be int32 tensors of the same length")
    i, j = i.contiguous(), j.contiguous()
    pairs = i.numel()
    dev = dx.residues.device
    mt = torch.empty(max(pairs, 1), dtype=torch.int32, device=dev)
    ln = torch.empty_like(mt)
    work = _work(work, lambda: max(nw_rescore_workspace_bytes(pairs), 16), dev, ValueError("work must be a 1-d uint8 tensor with unit stride"),
                 flat=True)
    _call(lib.da_dev_nw_rescore_pairs, dx.codes.data_ptr(), dx.offsets.data_ptr(), dx.n, dy.codes.data_ptr(), dy.offsets.data_ptr(), dy.n, i.data_ptr(),
          j.data_ptr(), pairs, mid, int(gap_open), int(gap_ext), mt.data_ptr(), ln.data_ptr(), work.data_ptr(), work.numel(), _stream())
    return mt[:pairs], ln[:pairs]


def lsh_nw_edges(sig, ds, n_hash, bands, rows, threshold, mh_threshold=0.0, matrix_name="BLOSUM62", gap_open=10, gap_ext=4, max_candidates=1 << 32,
                 capacity=None, work=None, index=None, sig_y=None, dy=None):
    """The NW identity on LSH candidates, resident signatures and resident encoded sequences in, a resident list out (da_dev_lsh_nw_edges):
    ``sig`` the signatures of ``ds`` (ds.codes filled by nw_encode) -> (i int32, j int32, matches int32, length int32), sorted by (i, j):
    the candidates of ``lsh_edges(sig, ..., mh_threshold)``, the diagonal included, whose ``matches / length >= threshold`` and > 0.  Two
    sets (da_dev_lsh_cross_nw_edges): pass ``index = lsh_index_build(sig_y, n_hash, bands, rows)``, ``sig_y`` and ``dy``; ``sig`` / ``ds``
    are then the queries x, and there is no diagonal.  ``capacity=None``: a first call counts, a second one fills; an int: one call, and at
    most that many edges are returned (``nw_lsh_last_route()["edges"]`` has the full number).  Synchronises the stream."""
    lib = _capi.load()
    cross = index is not None
    if cross and (sig_y is None or dy is None):
        raise ValueError("the two-set form needs index, sig_y and dy")
    if ds.codes is None or (cross and dy.codes is None):
        raise ValueError("call nw_encode on the sequences first")
    mid = _matrix_id(lib, matrix_name)
    dev = sig.device
    if cross:
        m, ld_x, n, ld_y, work = _lsh_cross_operands(index, sig, sig_y, n_hash, bands, work)
    else:
        n, ld = _sig_block(sig, n_hash)
        work = _lsh_work(work, n, bands, dev)
    got = ctypes.c_int64(0)

    def run(cap, ti, tj, tm, tl):
        if cross:
            _call(lib.da_dev_lsh_cross_nw_edges, index.data_ptr(), index.numel(), sig.data_ptr(), m, ld_x, sig_y.data_ptr(), n, ld_y, int(n_hash),
                  int(bands), int(rows), float(mh_threshold), int(max_candidates), ds.codes.data_ptr(), ds.offsets.data_ptr(), dy.codes.data_ptr(),
                  dy.offsets.data_ptr(), mid, int(gap_open), int(gap_ext), float(threshold), work.data_ptr(), work.numel(), ti, tj, tm, tl, cap,
                  ctypes.byref(got), _stream())
        else:
            _call(lib.da_dev_lsh_nw_edges, sig.data_ptr(), n, ld, int(n_hash), int(bands), int(rows), float(mh_threshold), int(max_candidates),
                  ds.codes.data_ptr(), ds.offsets.data_ptr(), mid, int(gap_open), int(gap_ext), float(threshold), work.data_ptr(), work.numel(),
                  ti, tj, tm, tl, cap, ctypes.byref(got), _stream())
        return got.value
    return _count_then_fill(run, capacity, dev, (torch.int32,) * 4)


def nw_knn_select(ptr, col, key, top, nnz=None, out=None):
    """``lsh_knn_select`` on 32-bit keys (da_dev_nw_knn_select), the selection of the NW-ranked LSH lists: ``key`` int32 (uint32 bit
    patterns over their whole range: value ranks) -> (idx int32 (n, top), key int32 (n, top)): per row the first ``top`` entries by (key
    descending as unsigned, column ascending), then -1 / 0.  Everything else as ``lsh_knn_select``."""
    lib = _capi.load()
    for t, name in ((ptr, "ptr"), (col, "col"), (key, "key")):
        _require_cuda(t, name)
    assert ptr.dtype == torch.int64 and col.dtype == torch.int32 and key.dtype == torch.int32
    assert ptr.is_contiguous() and col.is_contiguous() and key.is_contiguous() and col.numel() == key.numel()
    n = int(ptr.numel()) - 1
    nnz = int(col.numel()) if nnz is None else int(nnz)
    if not 0 <= nnz <= col.numel():
        raise ValueError("nnz must be in 0 .. col.numel()")
    t = _top(top)
    if out is None:
        idx, okey = _topk_out(n, top, torch.int32, ptr.device)
    else:
        idx, okey = out
        for o in (idx, okey):
            _require_cuda(o, "out")
            assert o.dim() == 2 and o.dtype == torch.int32 and o.shape[0] >= n and o.shape[1] >= t and o.stride(1) == 1
    _call(lib.da_dev_nw_knn_select, ptr.data_ptr(), nnz, col.data_ptr(), key.data_ptr(), n, int(top), idx.data_ptr(), idx.stride(0),
          okey.data_ptr(), okey.stride(0), _stream())
    return idx[:n, :t], okey[:n, :t]


def nw_rank_keys(i, j, matches, length, rank, max_len, r_min=1, one_set=True, n=0):
    """The rank-key step of the NW-ranked LSH lists on a caller's scored pairs (da_dev_nw_rank_keys): int32 device tensors ``i``, ``j``,
    ``matches``, ``length`` and the device rank table of ``nw_value_ranks(max_len)`` -> (key int32 (uint32 value ranks), keep uint8,
    diag_key int32 (n), totals int64 (2) = kept pairs, pairs outside the table).  keep = key >= r_min and key > 0; ``one_set``: a pair
    with i == j is not kept and its key goes to diag_key[i].  Asynchronous on the current stream."""
    lib = _capi.load()
    for t, name in ((i, "i"), (j, "j"), (matches, "matches"), (length, "length"), (rank, "rank")):
        _require_cuda(t, name)
        assert t.dtype == torch.int32 and t.is_contiguous()
    pairs = int(i.numel())
    assert j.numel() == pairs and matches.numel() == pairs and length.numel() == pairs
    assert rank.numel() >= (2 * int(max_len) + 1) * (int(max_len) + 1)
    dev = i.device
    key = torch.zeros(max(pairs, 1), dtype=torch.int32, device=dev)
    keep = torch.zeros(max(pairs, 1), dtype=torch.uint8, device=dev)
    diag = torch.zeros(max(int(n), 1), dtype=torch.int32, device=dev)
    totals = torch.zeros(2, dtype=torch.int64, device=dev)
    _call(lib.da_dev_nw_rank_keys, i.data_ptr(), j.data_ptr(), matches.data_ptr(), length.data_ptr(), pairs, rank.data_ptr(), int(max_len),
          int(r_min), 1 if one_set else 0, int(n), key.data_ptr(), keep.data_ptr(), diag.data_ptr(), totals.data_ptr(), _stream())
    return key[:pairs], keep[:pairs], diag[:int(n)], totals


def lsh_nw_knn(sig, ds, n_hash, bands, rows, top, rank, max_len, threshold=0.0, mh_threshold=0.0, matrix_name="BLOSUM62", gap_open=10, gap_ext=4,
               max_candidates=1 << 32, work=None):
    """The NW-ranked LSH nearest-neighbour lists, resident signatures and resident encoded sequences in, resident lists out
    (da_dev_lsh_nw_knn): ``sig`` the signatures of ``ds`` (ds.codes filled by nw_encode), ``rank`` the int32 device copy of the rank table of
    ``nw_value_ranks(max_len)``, max_len >= the longest sequence -> (idx int32 (n, top), key int32 (n, top), diag_key int32 (n)): value ranks
    as uint32 bit patterns, padding -1 / 0; value = values[rank].  ``nw_lsh_last_route()["edges"]`` has the number of real entries.
    Synchronises the stream."""
    lib = _capi.load()
    if ds.codes is None:
        raise ValueError("call nw_encode on the sequences first")
    mid = _matrix_id(lib, matrix_name)
    _require_cuda(rank, "rank")
    n, ld = _sig_block(sig, n_hash)
    work = _lsh_work(work, n, bands, sig.device)
    idx, key = _topk_out(n, top, torch.int32, sig.device)
    diag = torch.empty(max(n, 1), dtype=torch.int32, device=sig.device)
    _call(lib.da_dev_lsh_nw_knn, sig.data_ptr(), n, ld, int(n_hash), int(bands), int(rows), float(mh_threshold), int(max_candidates),
          ds.codes.data_ptr(), ds.offsets.data_ptr(), mid, int(gap_open), int(gap_ext), float(threshold), int(top), rank.data_ptr(), int(max_len),
          work.data_ptr(), work.numel(), idx.data_ptr(), key.data_ptr(), diag.data_ptr(), _stream())
    return idx[:n], key[:n], diag[:n]


def lsh_nw_cross_topk(index, sig_x, dx, sig_y, dy, n_hash, bands, rows, top, rank, max_len, threshold=0.0, mh_threshold=0.0, matrix_name="BLOSUM62",
                      gap_open=10, gap_ext=4, max_candidates=1 << 32, work=None):
    """The two-set form of ``lsh_nw_knn`` (da_dev_lsh_cross_nw_topk): ``index = lsh_index_build(sig_y, n_hash, bands, rows)``; the queries
    ``sig_x`` / ``dx`` against ``sig_y`` / ``dy`` -> (idx int32 (m, top), key int32 (m, top)), x[i] as sequence1.  Synchronises the stream."""
    lib = _capi.load()
    if dx.codes is None or dy.codes is None:
        raise ValueError("call nw_encode on the sequences first")
    mid = _matrix_id(lib, matrix_name)
    _require_cuda(rank, "rank")
    m, ld_x, n, ld_y, work = _lsh_cross_operands(index, sig_x, sig_y, n_hash, bands, work)
    idx, key = _topk_out(m, top, torch.int32, sig_x.device)
    _call(lib.da_dev_lsh_cross_nw_topk, index.data_ptr(), index.numel(), sig_x.data_ptr(), m, ld_x, sig_y.data_ptr(), n, ld_y, int(n_hash), int(bands),
          int(rows), float(mh_threshold), int(max_candidates), dx.codes.data_ptr(), dx.offsets.data_ptr(), dy.codes.data_ptr(), dy.offsets.data_ptr(),
          mid, int(gap_open), int(gap_ext), float(threshold), int(top), rank.data_ptr(), int(max_len), work.data_ptr(), work.numel(), idx.data_ptr(),
          key.data_ptr(), _stream())
    return idx[:m], key[:m]


def nw_lsh_last_route():
    from .similarity import nw_lsh_last_route as route
    return route()


def mh_cross_last_route():
    """what this thread's last similarity_mh_cross call did: dict(m, n, unique_x, unique_y, dedup, plane_bits, plan_ms, codes_ms,
    k2_ms, lists_ms, expand_ms)"""
    m, n, ux, uy = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    t, b = ctypes.c_int(0), ctypes.c_int(0)
    ms = (ctypes.c_double * 5)()
    _capi.check(_capi.load().da_mh_cross_last_route(ctypes.addressof(m), ctypes.addressof(n), ctypes.addressof(ux), ctypes.addressof(uy),
                                                    ctypes.addressof(t), ctypes.addressof(b), ctypes.addressof(ms)))
    return {"m": m.value, "n": n.value, "unique_x": ux.value, "unique_y": uy.value, "dedup": t.value == 1, "plane_bits": b.value,
            "plan_ms": ms[0], "codes_ms": ms[1], "k2_ms": ms[2], "lists_ms": ms[3], "expand_ms": ms[4]}


def mh_last_route():
    """what this thread's last similarity_mh call did: dict(n, unique, dedup, plane_bits, plan_ms, codes_ms, k2_ms, gather_ms, expand_ms, border_ms)"""
    n, u, t, b = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int(0)
    ms = (ctypes.c_double * 6)()
    _capi.check(_capi.load().da_mh_last_route(ctypes.addressof(n), ctypes.addressof(u), ctypes.addressof(t), ctypes.addressof(b),
                                              ctypes.addressof(ms)))
    # route 1 = duplicate-collapsing, 2 = sparse (signatures rarely agree: matching incidences bucketed per tile; then `unique` carries their
    # number, k2_ms the bucket phase and expand_ms the tile pass), 0 = the direct kernels
    # 4 = route 1 with the ROW expansion (k_expand_stream: no gathered copy; gather_ms = the copy lists, expand_ms = that kernel, border_ms = 0)
    # 3 = route 1 in its pipelined form (table compared band by band on a side stream while finished row bands are expanded: k2_ms is the
    # compare's span, gather_ms / expand_ms are sums over the chunk launches, all three overlap)
    sparse = t.value == 2
    ch, el = ctypes.c_int(0), ctypes.c_int(0)
    _capi.check(_capi.load().da_mh_last_route_chunks(ctypes.addressof(ch), ctypes.addressof(el)))
    rare, pb0 = ctypes.c_int64(0), ctypes.c_int(0)
    _capi.check(_capi.load().da_mh_last_route_split(ctypes.addressof(rare), ctypes.addressof(pb0)))
    # heavy / rare split of the column dictionaries: 8 dense planes + `rare_pairs` incidences added from lists (plane_bits_without: what it replaced)
    return {"split": rare.value >= 0, "rare_pairs": max(rare.value, 0), "plane_bits_without": pb0.value,
            "chunks": ch.value, "expand_launches": el.value, "n": n.value, "unique": n.value if sparse else u.value, "dedup": t.value in (1, 3, 4, 5), "pipelined": t.value in (3, 5),
            "expansion": {1: "tiles", 3: "tiles, pipelined", 4: "rows", 5: "rows, pipelined"}.get(t.value, ""), "sparse": sparse,
            "sparse_pairs": u.value if sparse else 0, "plane_bits": b.value, "plan_ms": ms[0], "codes_ms": ms[1],
            "k2_ms": ms[2], "gather_ms": ms[3], "expand_ms": ms[4], "border_ms": ms[5]}


class UniquePlan:
    """da_dev_unique_plan: byte-identical strings collapsed.  Keeps the workspace tensor the plan's device pointers point into."""

    def __init__(self, bytes_t, offsets_t, n, total):
        lib = _capi.load()
        _require_cuda(bytes_t, "sequence bytes")
        nbytes = int(lib.da_dev_unique_plan_bytes(int(n), int(total)))
        self.work = torch.empty(nbytes, dtype=torch.uint8, device=bytes_t.device)
        self.c = _capi.DaUniquePlan()
        self.c.struct_size = ctypes.sizeof(_capi.DaUniquePlan)
        _call(lib.da_dev_unique_plan, bytes_t.data_ptr(), offsets_t.data_ptr(), int(n), int(total), self.work.data_ptr(), nbytes,
                                           ctypes.addressof(self.c), _stream())
        self.n, self.unique = int(self.c.n), int(self.c.unique)

    def ptr(self):
        return ctypes.addressof(self.c)


def shards_to_table(gathered, ld_g, n, world, value_bits, out=None):
    """gathered MinHash shards (uint16 blocks: value_bits = 0; packed: their bit count) -> symmetric uint16 table [n][ld]"""
    ld = -(-int(n) // 8) * 8
    if out is None:
        out = torch.empty((int(n), ld), dtype=torch.int16, device=gathered.device)
    _call(_capi.load().da_dev_shards_to_table, gathered.data_ptr(), int(ld_g), int(n), int(world), int(value_bits), out.data_ptr(),
                                                    out.stride(0), _stream())
    return out


def nw_unique_rows(plan, max_len, matrix_name, gap_open, gap_ext, rank, world, out_rows):
    """rank `rank` of `world`'s cyclic 128-row units of the ordered unique NW table into out_rows (int16 [Q * 128][ld >= unique])"""
    lib = _capi.load()
    mid = _matrix_id(lib, matrix_name)
    _call(lib.da_dev_nw_unique_rows, plan.ptr(), int(max_len), mid, int(gap_open), int(gap_ext), int(rank), int(world),
                                          out_rows.data_ptr(), out_rows.stride(0), _stream())


def expand_workspace_bytes(n, unique, is_nw, n_hash=0, nw_max_len=0):
    return int(_capi.load().da_dev_expand_workspace_bytes(int(n), int(unique), 1 if is_nw else 0, int(n_hash), int(nw_max_len)))


def expand_unique(table, plan, is_nw, n_hash, nw_max_len, out, table_world=1, work=None):
    """dense float64 n x n from the table of the unique strings (da_dev_expand_unique)"""
    work = _work(work, lambda: expand_workspace_bytes(plan.n, plan.unique, is_nw, n_hash, nw_max_len), table.device)
    _call(_capi.load().da_dev_expand_unique, table.data_ptr(), table.stride(0), int(table_world), plan.ptr(), 1 if is_nw else 0,
                                                  int(n_hash), int(nw_max_len), work.data_ptr(), work.numel(), out.data_ptr(), out.stride(0),
                                                  _stream())
    return out


def nw_last_route():
    """what this thread's last whole-matrix NW call did: dict(n, unique, dedup, plan_ms, dp_ms, expand_ms)"""
    n, u, t = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int(0)
    ms = (ctypes.c_double * 3)()
    _capi.check(_capi.load().da_nw_last_route(ctypes.addressof(n), ctypes.addressof(u), ctypes.addressof(t), ctypes.addressof(ms)))
    return {"n": n.value, "unique": u.value, "dedup": bool(t.value), "plan_ms": ms[0], "dp_ms": ms[1], "expand_ms": ms[2]}
