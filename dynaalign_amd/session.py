"""Device-resident MinHash session for the caller's recursion.

clusterbreak re-calls ``sim_fn`` on every subset it splits off (reference R/clusterbreak.R:203-259,
``:246-254``), and each call of the reference re-uploads, re-hashes and re-seeds.  A signature does not
depend on which other sequences are in the call, so with the hash seed held fixed the signatures of the
full set can stay in HBM and a recursion level only needs K1b (codes of the subset's rows) + K2:

    s = MinHashSession(sequences, k=4, n_hash=500, seed=12345)      # upload + K1 once
    S = s.similarity(idx)                                           # == similarityMH(sequences[idx], 4, 500, seed=12345)
    thr, i, j, w = s.edges(idx, thresh_p=0.8)                       # == similarityMH_edges(sequences[idx], ...)
    R = s.cross(new, idx)                                           # == similarityMH_cross(new, sequences[idx], 4, 500, seed=12345)
    i, v = s.cross_topk(new, 10, idx)                               # == similarityMH_cross_topk(new, sequences[idx], 4, 500, 10, seed=12345)
    thr, ptr, j, w = s.cross_edges(new, 0.99, idx=idx)              # == similarityMH_cross_edges(new, sequences[idx], 4, 500, 0.99, seed=12345) as CSR
    i, v = s.knn(10, idx)                                           # == similarityMH_knn(sequences[idx], 4, 500, 10, seed=12345)
    thr, m, ptr, adj, codes, loops, values = s.knn_csr(idx, 10)     # the kNN graph of those lists as CSR (== similarityMH_knn_edges(...))
    member, c = s.lsh_components(12, 4, 0.5, idx)                   # == similarityMH_lsh_components(sequences[idx], 4, 48, 12, 4, 0.5, seed=12345) at n_hash = 48
    member, c = s.components(idx, thresh_p=0.8)                     # == components_dense on s.edges(idx, thresh_p=0.8), the graph kept on the device
    thr, i, j, w = s.lsh_edges(12, 4, 0.5, idx)                     # == similarityMH_lsh_edges(sequences[idx], 4, 48, 12, 4, 0.5, seed=12345) at n_hash = 48
    i, v = s.lsh_knn(12, 4, 10, idx)                                # == similarityMH_lsh_knn(sequences[idx], 4, 48, 12, 4, 10, seed=12345) at n_hash = 48
    thr, ptr, j, w = s.lsh_cross_edges(new, 12, 4, 0.5, idx)        # == similarityMH_lsh_cross_edges(new, sequences[idx], 4, 48, 12, 4, 0.5, seed=12345) as CSR
    i, v = s.lsh_cross_topk(new, 12, 4, 10, idx)                    # == similarityMH_lsh_cross_topk(new, sequences[idx], 4, 48, 12, 4, 10, seed=12345)
    st = s.stats(idx)                                               # == similarityMH_stats(sequences[idx], 4, 500, seed=12345)

The only difference to calling the reference per level is the random stream (the reference draws fresh
seeds per call, src/minHash.cpp:73,137); the contract -- MinHash estimates under one hash family -- holds.
The recursion itself (and its Louvain step) is restated in dynaalign_amd/clusterbreak.py, which drives this session.
"""
import numpy as np
import torch

from . import _capi, device
from .similarity import SimilarityMatrix, hash_family_seeds, pack_sequences, quantile_type7, stats_from_records, _resolve_seed


class MinHashSession:
    def __init__(self, sequences, k=4, n_hash=50, *, seed=None, device_name="cuda", reserve=True):
        res, off = pack_sequences(sequences)
        self.n, self.k, self.n_hash = len(off) - 1, int(k), int(n_hash)
        self.seed = _resolve_seed(seed)
        self.seeds = hash_family_seeds(self.seed, self.n_hash) if self.n_hash > 0 else np.zeros(1, np.uint32)
        self.ds = device.DeviceSequences(res, off, device_name)
        # validation (order and messages of the reference) happens in the library call
        self.sig, _ = device.minhash_signatures(self.ds, self.k, self.n_hash, self.seeds, want_planes=False)
        self._lsh_indexes = {}               # (bands, rows, idx is None) -> (idx, signatures, rows, index): lsh_index
        if reserve and self.n >= 2:
            # the first recursion level needs an n x n uint16 count matrix (20 GB at n = 100k) and a fresh hipMalloc of that size
            # costs 0.3 - 2.3 s depending on the box: take it here once, hand it to the caching allocator, and every level finds it
            try:
                free_b, _ = torch.cuda.mem_get_info(self.sig.device)
                if 2 * self.n * self.n <= free_b // 2:
                    torch.empty(self.n * self.n, dtype=torch.int16, device=self.sig.device)
            except RuntimeError:
                pass

    def _subset(self, idx):
        if idx is None:
            return self.sig, self.n
        idx_t = torch.as_tensor(np.ascontiguousarray(idx, np.int64), device=self.sig.device)
        if idx_t.numel() == 0:
            _capi.check(_capi.DA_ERR_EMPTY_INPUT)
        return self.sig.index_select(0, idx_t).contiguous(), int(idx_t.numel())

    def planes(self, idx=None):
        sig, m = self._subset(idx)
        return device.mh_planes(sig, m, self.n_hash), m

    def similarity(self, idx=None):
        """dense float64 matrix of the subset (host copy), rows/columns in the order of idx"""
        planes, m = self.planes(idx)
        out = device.mh_compare(planes, m, self.n_hash)
        return SimilarityMatrix(out.cpu().numpy())

    def _joint_operand(self, sequences, idx):
        """The compare operand of new sequences against the resident set (or its subset idx): K1 on the new strings under the session's
        seeds, ONE dictionary over [new ; filler ; resident[idx]] -- the new rows padded to a multiple of 128 with rows that repeat real
        ones, so the rectangle's origins are tile-aligned.  -> (planes, m, m_pad, n): the rectangle is rows [0, m) x columns
        [m_pad, m_pad + n) of the (m_pad + n)-row problem."""
        res, off = pack_sequences(sequences)
        m = len(off) - 1
        if m == 0:
            _capi.check(_capi.DA_ERR_EMPTY_INPUT)
        new = device.DeviceSequences(res, off, self.sig.device)
        sig_new, _ = device.minhash_signatures(new, self.k, self.n_hash, self.seeds, want_planes=False)
        sig_res, n = self._subset(idx)
        m_pad = -(-m // 128) * 128
        if m_pad + n > 131068 >= m + n:       # keep the dictionary rather than the alignment, as da_dev_similarity_mh_cross does
            m_pad = m
        joint = torch.empty((m_pad + n, self.sig.shape[1]), dtype=torch.int32, device=self.sig.device)
        joint[:m] = sig_new[:m]
        if m_pad > m:
            joint[m:m_pad] = sig_new[torch.arange(m_pad - m, device=self.sig.device) % m]
        joint[m_pad:] = sig_res[:n]
        return device.mh_planes(joint, m_pad + n, self.n_hash), m, m_pad, n

    def cross(self, sequences, idx=None):
        """New sequences against the resident set (or its subset idx): the (m, len(idx)) float64 matrix
        similarityMH_cross(sequences, resident[idx], k, n_hash, seed=self.seed): the joint operand (_joint_operand), then the
        rectangle compare."""
        planes, m, m_pad, n = self._joint_operand(sequences, idx)
        out = device.mh_compare_rect(planes, m_pad + n, self.n_hash, 0, m, m_pad, m_pad + n)
        return SimilarityMatrix(out.cpu().numpy()[:m, :n])

    def cross_topk(self, sequences, top=10, idx=None, block_bytes=1 << 30):
        """For every new sequence its `top` most similar resident sequences (or members of the subset idx), without the m x n matrix:
        (index, value) = similarityMH_cross_topk(sequences, resident[idx], k, n_hash, top, seed=self.seed) -- (m, top) int32 positions
        in idx (in the resident set when idx is None), by value descending then position ascending, and the (m, top) float64 values.
        top is clamped to the number of columns.  The rectangle is compared into uint16 counts in row blocks of block_bytes and each
        block goes through device.topk_rows."""
        planes, m, m_pad, n = self._joint_operand(sequences, idx)
        top = min(int(top), n)
        ld = -(-n // 8) * 8
        blk = min(max(block_bytes // (2 * ld) // 128 * 128, 128), m)
        buf = torch.empty((blk, ld), dtype=torch.int16, device=self.sig.device)
        out_i, out_k = [], []
        for b0 in range(0, m, blk):
            b1 = min(m, b0 + blk)
            cnt = device.mh_compare_rect(planes, m_pad + n, self.n_hash, b0, b1, m_pad, m_pad + n, _capi.DA_OUT_COMPACT, out=buf[:b1 - b0, :n])
            i, key = device.topk_rows(cnt, top, rank_bits=max(self.n_hash.bit_length(), 1))
            out_i.append(i)
            out_k.append(key)
        keys = torch.cat(out_k).contiguous()
        val = device.widen(keys, False, self.n_hash)                     # count / n_hash, the library's divide
        return torch.cat(out_i).cpu().numpy(), val.cpu().numpy()

    def cross_edges(self, sequences, thresh_p=0.8, threshold=None, idx=None, block_bytes=1 << 30):
        """The entries of cross(sequences, idx) that pass a threshold, without the m x n matrix, as CSR over the new sequences:
        (threshold, rowptr, j, w) device tensors -- int64 (m + 1), int32 positions in idx (in the resident set when idx is None), ascending
        within a row, and the float64 similarities -- of the entries with R >= threshold and R > 0, as
        similarityMH_cross_edges(sequences, resident[idx], k, n_hash, thresh_p, threshold=threshold, seed=self.seed).  threshold=None: the
        type-7 quantile thresh_p of all m * n entries (a histogram pass over the row blocks first; a rectangle of several blocks is compared
        twice).  The rectangle is compared into uint16 counts in row blocks of block_bytes; each goes through device.threshold_rows."""
        planes, m, m_pad, n = self._joint_operand(sequences, idx)
        nbins = self.n_hash + 1
        values = np.arange(nbins, dtype=np.float64) / np.float64(self.n_hash)          # src/minHash.cpp:174
        ld = -(-n // 8) * 8
        blk = min(max(block_bytes // (2 * ld) // 128 * 128, 128), m)
        buf = torch.empty((blk, ld), dtype=torch.int16, device=self.sig.device)

        def block(b0):
            b1 = min(m, b0 + blk)
            return device.mh_compare_rect(planes, m_pad + n, self.n_hash, b0, b1, m_pad, m_pad + n, _capi.DA_OUT_COMPACT, out=buf[:b1 - b0, :n])
        kept_block = None
        if threshold is None:
            if not 0.0 <= float(thresh_p) <= 1.0:
                raise _capi.DynaAlignError(_capi.DA_ERR_BAD_ARG, "thresh_p must be in [0, 1]")
            hist = torch.zeros(nbins, dtype=torch.int64, device=self.sig.device)
            for b0 in range(0, m, blk):
                kept_block = block(b0)
                hist += device.rect_histogram(kept_block, nbins)
            thr = quantile_type7(hist.cpu().numpy().astype(np.uint64), values, float(thresh_p))
            if blk < m:
                kept_block = None
        else:
            thr = float(threshold)
            if thr != thr:
                raise _capi.DynaAlignError(_capi.DA_ERR_BAD_ARG, "the threshold must not be NaN")
        keep = torch.from_numpy(((values > 0.0) & (values >= thr)).astype(np.uint8)).to(self.sig.device)
        ptrs, js, keys, base = [], [], [], 0
        for b0 in range(0, m, blk):
            rp, j, key = device.threshold_rows(kept_block if kept_block is not None else block(b0), keep)
            ptrs.append(rp[:-1] + base)
            js.append(j)
            keys.append(key)
            base += int(rp[-1].item())
        ptrs.append(torch.tensor([base], dtype=torch.int64, device=self.sig.device))
        key_all = torch.cat(keys).contiguous()
        w = device.widen(key_all, False, self.n_hash) if base else torch.empty(0, dtype=torch.float64, device=self.sig.device)
        return thr, torch.cat(ptrs), torch.cat(js), w

    def _knn_lists(self, idx, top, block_bytes):
        """device tensors (idx int32 (m, top), key int16 (m, top)) of the subset's nearest-neighbour lists, and m: subset -> planes -> row
        blocks of the square problem (rows [b0, b1) x columns [0, m)) -> device.topk_rows with self_col0 = b0"""
        planes, m = self.planes(idx)
        if m < 2:
            raise _capi.DynaAlignError(_capi.DA_ERR_BAD_ARG, "a nearest neighbour needs a second sequence")
        top = min(int(top), m - 1)
        ld = -(-m // 8) * 8
        blk = min(max(block_bytes // (2 * ld) // 128 * 128, 128), m)
        buf = torch.empty((blk, ld), dtype=torch.int16, device=self.sig.device)
        out_i, out_k = [], []
        for b0 in range(0, m, blk):
            b1 = min(m, b0 + blk)
            cnt = device.mh_compare_rect(planes, m, self.n_hash, b0, b1, 0, m, _capi.DA_OUT_COMPACT, out=buf[:b1 - b0, :m])
            i, key = device.topk_rows(cnt, top, rank_bits=max(self.n_hash.bit_length(), 1), self_col0=b0)
            out_i.append(i)
            out_k.append(key)
        return torch.cat(out_i).contiguous(), torch.cat(out_k).contiguous(), m

    def knn(self, top=10, idx=None, block_bytes=1 << 30):
        """For every resident sequence (or member of the subset idx) its `top` most similar OTHER ones, without the matrix: (index, value) =
        similarityMH_knn(sequences[idx], k, n_hash, top, seed=self.seed) -- (m, top) int32 positions in idx, by value descending then
        position ascending, the row's own position left out, and the (m, top) float64 values.  top is clamped to m - 1.  The signatures are
        resident: a call is K1b on the subset, the square problem's rows in blocks of block_bytes as uint16 counts, and the self form of
        device.topk_rows on each block."""
        i, key, _ = self._knn_lists(idx, top, block_bytes)
        val = device.widen(key, False, self.n_hash)                      # count / n_hash, the library's divide
        return i.cpu().numpy(), val.cpu().numpy()

    def _csr_out(self, thr, got, ptr, adj, codes, loops, values, on_device):
        """the CSR of edges_csr / knn_csr / lsh_knn_csr: host copies, or with on_device the device tensors device.louvain_csr takes"""
        if on_device:
            return thr, got, ptr, adj, codes, loops, values
        return thr, got, ptr.cpu().numpy(), adj.cpu().numpy(), codes.cpu().numpy().view(np.uint16), loops.cpu().numpy().view(np.uint16), values

    def _min_code_threshold(self, codes, values):
        """the smallest off-diagonal weight kept (NaN when none), from the device codes"""
        if codes.numel() == 0:
            return float("nan")
        return float(values[int((codes.to(torch.int32) & 0xFFFF).min().item())])

    def knn_csr(self, idx=None, top=10, mode="union"):
        """The kNN graph of the subset (knn_graph of knn(top, idx) with the 1.0 diagonal) as the canonical symmetric CSR edges_csr returns --
        lists -> device.knn_edges -> device.edges_to_csr, all on the device: (threshold, n_edges, ptr, adj, codes, loop_codes, values) with
        weight of entry k = values[codes[k]]; n_edges counts i <= j entries, the diagonal included.  The threshold slot holds the smallest
        off-diagonal weight kept, NaN when none."""
        return self._knn_csr(idx, top, mode, False)

    def knn_csr_device(self, idx=None, top=10, mode="union"):
        """knn_csr with ptr, adj, codes and loop_codes left as device tensors (what device.louvain_csr takes): nothing but the threshold's
        code crosses to the host.  (knn_csr keeps its parameter list; edges_csr spells this on_device=True.)"""
        return self._knn_csr(idx, top, mode, True)

    def _knn_csr(self, idx, top, mode, on_device):
        i, key, m = self._knn_lists(idx, top, 1 << 30)
        ei, ej, ev, got = device.knn_edges(i, key, mode, is_nw=False, self_code=self.n_hash, loops=True)
        ptr, adj, codes, loops = device.edges_to_csr(ei, ej, ev, got, m)
        values = np.arange(self.n_hash + 1, dtype=np.float64) / self.n_hash           # src/minHash.cpp:174
        return self._csr_out(self._min_code_threshold(codes, values), got, ptr, adj, codes, loops, values, on_device)

    def edges_csr(self, idx=None, thresh_p=0.8, on_device=False):
        """The thresholded graph of the subset as the canonical symmetric CSR clusterbreak.louvain_csr takes -- sorted ON THE DEVICE
        (da_dev_edges_to_csr), so neither a host-side sort nor 16 bytes per edge: (threshold, n_edges, ptr, adj, codes, loop_codes,
        values) with weight of entry k = values[codes[k]]; n_edges counts i <= j entries like `edges`.  on_device=True: ptr, adj, codes and
        loop_codes stay device tensors (what device.louvain_csr takes) and the graph is not copied to the host."""
        import os, sys, time
        trace = os.environ.get("DYNAALIGN_TRACE") is not None
        marks = [("start", time.perf_counter())]

        def mark(what):
            if trace:
                torch.cuda.synchronize()
                marks.append((what, time.perf_counter()))
        planes, m = self.planes(idx)
        if m < 2:
            raise _capi.DynaAlignError(_capi.DA_ERR_BAD_ARG, "the threshold is a quantile of the strict upper triangle: need >= 2 sequences")
        mark("codes")
        cnt = device.mh_compare(planes, m, self.n_hash, kind=_capi.DA_OUT_COMPACT)
        mark("compare")
        nbins = self.n_hash + 1
        hist = device.upper_histogram(cnt, m, nbins).cpu().numpy().astype(np.uint64)
        values = np.arange(nbins, dtype=np.float64) / self.n_hash           # src/minHash.cpp:174
        thr = quantile_type7(hist, values, thresh_p)
        keep = (~(values < thr)) & (np.arange(nbins) != 0)
        cap = int(hist[keep].sum()) + m
        mark("histogram + quantile")
        ei, ej, ev, c = device.extract_edges(cnt, m, keep, cap)
        got = int(c.item())
        assert got == cap, (got, cap)
        del cnt
        mark("extract")
        ptr, adj, codes, loops = device.edges_to_csr(ei, ej, ev, got, m)
        mark("edges -> CSR")
        out = self._csr_out(thr, got, ptr, adj, codes, loops, values, on_device)
        mark("CSR kept on the device" if on_device else "device -> host")
        if trace and m >= 20000:
            print("[dynaalign] edges_csr m=%d: %s" % (m, ", ".join("%s %.1f ms" % (w, (t - marks[i][1]) * 1e3)
                                                                    for i, (w, t) in enumerate(marks[1:]))), file=sys.stderr)
        return out

    def edges(self, idx=None, thresh_p=0.8, sort=True):
        """(threshold, i, j, weight) of the subset after clusterbreak's quantile threshold, i <= j positions in idx;
        sort=False leaves the edges in the order the device appended them (da_louvain canonicalises anyway)"""
        planes, m = self.planes(idx)
        if m < 2:
            raise _capi.DynaAlignError(_capi.DA_ERR_BAD_ARG, "the threshold is a quantile of the strict upper triangle: need >= 2 sequences")
        cnt = device.mh_compare(planes, m, self.n_hash, kind=_capi.DA_OUT_COMPACT)
        nbins = self.n_hash + 1
        hist = device.upper_histogram(cnt, m, nbins).cpu().numpy().astype(np.uint64)
        values = np.arange(nbins, dtype=np.float64) / self.n_hash           # src/minHash.cpp:174
        thr = quantile_type7(hist, values, thresh_p)
        keep = (~(values < thr)) & (np.arange(nbins) != 0)
        cap = int(hist[keep].sum()) + m
        ei, ej, ev, c = device.extract_edges(cnt, m, keep, cap)
        got = int(c.item())
        assert got == cap, (got, cap)
        ei, ej, ev = ei[:got].cpu().numpy(), ej[:got].cpu().numpy(), ev[:got].cpu().numpy().view(np.uint16)
        if not sort:
            return thr, ei, ej, values[ev]
        order = np.lexsort((ej, ei))
        return thr, ei[order], ej[order], values[ev[order]]

    def lsh_edges(self, bands, rows, threshold, idx=None, max_candidates=1 << 32):
        """``(threshold, i, j, w)`` == similarityMH_lsh_edges(sequences[idx], k, n_hash, bands, rows, threshold, seed=session.seed), from the
        resident signatures: bucketing, candidate verification and the (i, j) sort on the device, only the edge list crosses to the host."""
        sig, m = self._subset(idx)
        ei, ej, ec = device.lsh_edges(sig[:m], self.n_hash, bands, rows, threshold, max_candidates=max_candidates)
        c = ec.cpu().numpy().view(np.uint16).astype(np.float64)
        return float(threshold), ei.cpu().numpy(), ej.cpu().numpy(), c / np.float64(self.n_hash)

    def lsh_components(self, bands, rows, threshold, idx=None, max_candidates=1 << 32):
        """``(membership, n_components)`` == similarityMH_lsh_components(sequences[idx], k, n_hash, bands, rows, threshold, seed=session.seed),
        from the resident signatures: the components of `lsh_edges` for the same arguments, without the edge list -- n labels cross to the
        host.  Positions are those in idx."""
        sig, m = self._subset(idx)
        return device.lsh_components(sig[:m], self.n_hash, bands, rows, threshold, max_candidates=max_candidates)

    def components(self, idx=None, thresh_p=0.8):
        """``(membership, n_components)``: the connected components of the graph `edges` (idx, thresh_p) returns -- single-linkage groups at
        the quantile threshold -- by `device.components_csr` on the tensors of ``edges_csr(idx, thresh_p, on_device=True)``: the graph
        never leaves the device."""
        _, _, ptr, adj, _, _, _ = self.edges_csr(idx, thresh_p, on_device=True)
        return device.components_csr(ptr, adj, symmetric=True)

    def lsh_knn(self, bands, rows, top=10, idx=None, threshold=0.0, max_candidates=1 << 32):
        """``(idx, val)`` == similarityMH_lsh_knn(sequences[idx], k, n_hash, bands, rows, top, threshold=threshold, seed=session.seed), from the
        resident signatures: bucketing, candidate verification and the per-row selection on the device; positions are those in idx, the
        padding is -1 / 0.0.  ``top`` is not clamped to the subset's size."""
        sig, m = self._subset(idx)
        i, key = device.lsh_knn(sig[:m], self.n_hash, bands, rows, top, threshold=threshold, max_candidates=max_candidates)
        val = device.widen(key.contiguous(), False, self.n_hash)         # count / n_hash, the library's divide; the padding's 0 gives 0.0
        return i.cpu().numpy(), val.cpu().numpy()

    def lsh_knn_csr(self, bands, rows, idx=None, top=10, mode="union"):
        """The kNN graph of lsh_knn(bands, rows, top, idx) with the 1.0 diagonal as the canonical symmetric CSR knn_csr returns -- lists ->
        device.knn_edges (which skips the padding) -> device.edges_to_csr, all on the device: (threshold, n_edges, ptr, adj, codes,
        loop_codes, values).  What ``clusterbreak(session=, knn=, knn_lsh=(bands, rows))`` clusters on."""
        return self._lsh_knn_csr(bands, rows, idx, top, mode, False)

    def lsh_knn_csr_device(self, bands, rows, idx=None, top=10, mode="union"):
        """lsh_knn_csr with the CSR left in device tensors, as knn_csr_device"""
        return self._lsh_knn_csr(bands, rows, idx, top, mode, True)

    def _lsh_knn_csr(self, bands, rows, idx, top, mode, on_device):
        sig, m = self._subset(idx)
        i, key = device.lsh_knn(sig[:m], self.n_hash, bands, rows, top)
        ei, ej, ev, got = device.knn_edges(i, key, mode, is_nw=False, self_code=self.n_hash, loops=True)
        ptr, adj, codes, loops = device.edges_to_csr(ei, ej, ev, got, m)
        values = np.arange(self.n_hash + 1, dtype=np.float64) / self.n_hash           # src/minHash.cpp:174
        return self._csr_out(self._min_code_threshold(codes, values), got, ptr, adj, codes, loops, values, on_device)

    def _lsh_index_entry(self, bands, rows, idx):
        """(signatures of the indexed rows, their number, the index) for lsh_index's key; an idx subset is kept until another one is asked for"""
        bands, rows = int(bands), int(rows)
        cache = self._lsh_indexes
        key = (bands, rows, idx is None)
        idx_h = None if idx is None else np.ascontiguousarray(idx, np.int64).copy()
        kept = cache.get(key)
        if kept is not None and (idx is None or np.array_equal(kept[0], idx_h)):
            return kept[1:]
        sig, n = self._subset(idx_h)
        sig = sig[:n]
        cache[key] = (idx_h, sig, n, device.lsh_index_build(sig, self.n_hash, bands, rows))
        return cache[key][1:]

    def lsh_index(self, bands, rows, idx=None):
        """The LSH bucket index of the resident set (or its subset idx) for lsh_cross_edges / lsh_cross_topk: the device buffer of
        device.lsh_index_build, built once per (bands, rows, idx is None) and kept -- a second query against the same session neither
        rebuilds nor re-sorts it.  One subset index is kept per (bands, rows): asking for another idx replaces it."""
        return self._lsh_index_entry(bands, rows, idx)[2]

    def _query_signatures(self, sequences):
        res, off = pack_sequences(sequences)
        m = len(off) - 1
        if m == 0:
            _capi.check(_capi.DA_ERR_EMPTY_INPUT)
        new = device.DeviceSequences(res, off, self.sig.device)
        sig_new, _ = device.minhash_signatures(new, self.k, self.n_hash, self.seeds, want_planes=False)
        return sig_new[:m], m

    def lsh_cross_edges(self, sequences, bands, rows, threshold, idx=None, max_candidates=1 << 32):
        """New sequences against the resident set (or its subset idx) through the kept LSH index, as CSR over the new sequences like
        cross_edges: (threshold, rowptr, j, w) device tensors -- int64 (m + 1), int32 positions in idx (in the resident set when idx is
        None), ascending within a row, and the float64 similarities -- of similarityMH_lsh_cross_edges(sequences, resident[idx], k, n_hash,
        bands, rows, threshold, seed=self.seed).  A call is K1 on the new strings, a probe of the index and the compare of the pairs that
        share a bucket."""
        sig_y, n, index = self._lsh_index_entry(bands, rows, idx)
        sig_x, m = self._query_signatures(sequences)
        ei, ej, ec = device.lsh_cross_edges(index, sig_x, sig_y, self.n_hash, bands, rows, threshold, max_candidates=max_candidates)
        rowptr = torch.zeros(m + 1, dtype=torch.int64, device=self.sig.device)
        if ei.numel():
            rowptr[1:] = torch.cumsum(torch.bincount(ei.to(torch.int64), minlength=m), 0)
            w = device.widen(ec.contiguous(), False, self.n_hash)            # count / n_hash, the library's divide
        else:
            w = torch.empty(0, dtype=torch.float64, device=self.sig.device)
        return float(threshold), rowptr, ej, w

    def lsh_cross_topk(self, sequences, bands, rows, top=10, idx=None, threshold=0.0, max_candidates=1 << 32):
        """``(idx, val)`` == similarityMH_lsh_cross_topk(sequences, resident[idx], k, n_hash, bands, rows, top, threshold=threshold,
        seed=self.seed) through the kept LSH index: (m, top) int32 positions in idx and the (m, top) float64 values as cross_topk returns
        them, but a row with fewer candidates is padded with -1 / 0.0 and ``top`` is not clamped to the number of columns."""
        sig_y, n, index = self._lsh_index_entry(bands, rows, idx)
        sig_x, m = self._query_signatures(sequences)
        i, key = device.lsh_cross_topk(index, sig_x, sig_y, self.n_hash, bands, rows, top, threshold=threshold, max_candidates=max_candidates)
        val = device.widen(key.contiguous(), False, self.n_hash)         # count / n_hash, the library's divide; the padding's 0 gives 0.0
        return i.cpu().numpy(), val.cpu().numpy()

    def stats(self, idx=None):
        """compute_similarity_stats of the subset's similarity matrix without that matrix on the host (``SimilarityStats``, positions in
        idx), as similarityMH_stats(sequences[idx], k, n_hash, seed=self.seed): the uint16 counts, the histogram of their strict upper
        triangle, and every row's extremes with their first columns (device.upper_extrema)."""
        planes, m = self.planes(idx)
        if m < 2:
            raise _capi.DynaAlignError(_capi.DA_ERR_BAD_ARG, "the statistics are over the strict upper triangle: need >= 2 sequences")
        cnt = device.mh_compare(planes, m, self.n_hash, kind=_capi.DA_OUT_COMPACT)
        nbins = self.n_hash + 1
        hist = device.upper_histogram(cnt, m, nbins)
        rec = device.upper_extrema(cnt, m)
        values = np.arange(nbins, dtype=np.float64) / self.n_hash           # src/minHash.cpp:174
        return stats_from_records(hist.cpu().numpy().astype(np.uint64), values, rec.cpu().numpy())
