// nw_edges_long_kernels.hip -- the threshold step of the NW identity for sequences of up to 1024 residues, on 32-bit keys.
//
// The DP writes DA_OUT_PACK32 codes (matches << 16 | length).  With lengths up to 2048 a code no longer indexes a 65 536-entry value table,
// and the quantile is over VALUES (128/256 and 150/300 are one value), so the order key is the dense rank of a code's double value in the
// host table of da_nw_value_ranks:
//   1. k_codes_to_ranks: every code of a block is replaced by its rank (one lookup in the <= 8.4 MB table, resident in L2 / HBM);
//   2. k_rank_histogram: hist[rank] += occurrences, over the whole block or over the strict upper triangle of the square problem.  The
//      table has up to 1.3e6 bins -- far beyond LDS -- and clustered inputs put most pairs on a few of them, so equal keys are merged
//      before any atomic: within a wave by two rounds of leader election (one lane adds the population count of its key), within a
//      workgroup by a direct-mapped LDS cache of 4096 (tag, count) slots that is flushed once, and only what misses both goes to a
//      global atomic of its own;
//   3. the ordered compaction is k_threshold_count / k_threshold_emit (rect_edges_kernels.hip) on uint32 keys with the KeepRanks policy:
//      the keep decision is one compare, rank >= r_min; the mask is the rectangle or the upper triangle INCLUDING the diagonal.
// Rows are read through KeyRow<uint32_t> (row_keys.hpp): every ld and 4-byte-aligned base works.
#include "da_common.hpp"
#include "row_keys.hpp"

#include <algorithm>

namespace da {
namespace {

constexpr int RK_THREADS = 256;
constexpr int RK_PER = KeyRow<uint32_t>::PER;
constexpr int RK_WAVE_KEYS = 64 * RK_PER;      // what one wave takes per step of the histogram
constexpr int RK_CACHE = 4096;                 // slots of the workgroup's (tag, count) cache: 32 KiB
constexpr uint32_t RK_EMPTY = 0xFFFFFFFFu;

// out[r][c] = rank[length * (max_len + 1) + matches] of code[r][c] = matches << 16 | length; a code outside the table's domain -> 0.
// In place allowed: every element is read and written by the same thread.
__global__ __launch_bounds__(RK_THREADS) void k_codes_to_ranks(const uint32_t *codes, int64_t n, int64_t ld, int max_len,
                                                               const uint32_t *__restrict__ rank, uint32_t *out, int64_t ld_out,
                                                               int64_t per_row, int64_t units) {
  const uint32_t ml = (uint32_t)max_len;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t r = u / per_row, c = (u - r * per_row) * RK_THREADS + threadIdx.x;
    if (c >= n) continue;
    const uint32_t code = codes[r * ld + c];
    const uint32_t mt = code >> 16, ln = code & 0xFFFFu;
    uint32_t v = 0;
    if (ln >= 1 && ln <= 2 * ml && mt <= ml && mt <= ln) v = rank[(size_t)ln * (ml + 1) + mt];
    out[r * ld_out + c] = v;
  }
}

// one key with multiplicity c into the workgroup's cache, or -- its slot taken by another key -- straight to the global histogram
__device__ __forceinline__ void hist_add(uint32_t *tag, uint32_t *cnt, unsigned long long *__restrict__ hist, uint32_t key, uint32_t c) {
  const uint32_t slot = (key * 2654435761u) >> 20;           // 12 bits: RK_CACHE slots
  const uint32_t old = atomicCAS(&tag[slot], RK_EMPTY, key);
  if (old == RK_EMPTY || old == key) atomicAdd(&cnt[slot], c);
  else atomicAdd(&hist[key], (unsigned long long)c);
}

// hist[v] += number of keys equal to v among the counted elements; keys >= nbins are ignored.  TRI: only elements with global column
// (col_begin + c) > global row (row_begin + r) are counted.  Persistent workgroups; the unit of work is 256 consecutive keys of one row per
// WAVE.  A workgroup sees fewer than 2^32 keys (the launcher's bound), so the 32-bit cache counts cannot wrap.
template <bool TRI>
__global__ __launch_bounds__(RK_THREADS) void k_rank_histogram(const uint32_t *__restrict__ keys, int64_t n, int64_t ld, uint32_t nbins,
                                                               unsigned long long *__restrict__ hist, int64_t per_row, int64_t units,
                                                               int64_t row_begin, int64_t col_begin) {
  __shared__ uint32_t tag[RK_CACHE];
  __shared__ uint32_t cnt[RK_CACHE];
  static_assert(RK_CACHE == 1 << 12, "hist_add takes the top 12 bits of the hash");
  for (int s = threadIdx.x; s < RK_CACHE; s += RK_THREADS) { tag[s] = RK_EMPTY; cnt[s] = 0; }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (RK_THREADS / 64);
  uint32_t k[RK_PER];
  for (int64_t u = (int64_t)blockIdx.x * (RK_THREADS / 64) + (threadIdx.x >> 6); u < units; u += nwaves) {
    const int64_t rr = u / per_row, c0 = (u - rr * per_row) * RK_WAVE_KEYS;
    // first counted local column of this row: global column > global row
    const int64_t first = TRI ? row_begin + rr + 1 - col_begin : 0;
    if (TRI && c0 + RK_WAVE_KEYS <= first) continue;         // wave-uniform: the whole unit lies at or below the diagonal
    const uint32_t *row = keys + rr * ld;
    const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    const int64_t j0 = c0 + (int64_t)lane * RK_PER;
    const int nv = KeyRow<uint32_t>::load(row, j0, n, vec, k);
#pragma unroll
    for (int e = 0; e < RK_PER; ++e) {
      const uint32_t v = k[e];
      bool pend = e < nv && v < nbins && (!TRI || j0 + e >= first);
      // two rounds: the first pending lane's key is added once for all the lanes that hold it
#pragma unroll
      for (int round = 0; round < 2; ++round) {
        const unsigned long long act = __ballot(pend);
        if (!act) break;
        const int leader = __ffsll((long long)act) - 1;
        const uint32_t lk = (uint32_t)__shfl((int)v, leader);
        const bool same = pend && v == lk;
        const unsigned long long grp = __ballot(same);
        if (lane == leader) hist_add(tag, cnt, hist, lk, (uint32_t)__popcll(grp));
        if (same) pend = false;
      }
      if (pend) hist_add(tag, cnt, hist, v, 1u);
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < RK_CACHE; s += RK_THREADS)
    if (cnt[s]) atomicAdd(&hist[tag[s]], (unsigned long long)cnt[s]);
}

}  // namespace

int launch_nw_codes_to_ranks(const uint32_t *d_codes, int64_t rows, int64_t n, int64_t ld, int max_len, const uint32_t *d_rank, uint32_t *d_out,
                             int64_t ld_out, hipStream_t stream) {
  if (rows <= 0 || n <= 0) return DA_OK;
  int rc;
  if ((rc = block_shape_ok(rows, n)) != DA_OK) return rc;
  const int64_t per_row = ceil_div(n, RK_THREADS), units = rows * per_row;
  const unsigned grid = (unsigned)std::min<int64_t>(units, 256 * 32);
  hipLaunchKernelGGL(k_codes_to_ranks, dim3(grid), dim3(RK_THREADS), 0, stream, d_codes, n, ld, max_len, d_rank, d_out, ld_out, per_row, units);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

int launch_rank_histogram(const uint32_t *d_keys, int64_t rows, int64_t n, int64_t ld, int64_t nbins, unsigned long long *d_hist, bool triangle,
                          int64_t row_begin, int64_t col_begin, hipStream_t stream) {
  if (rows <= 0 || n <= 0) return DA_OK;
  int rc;
  if ((rc = block_shape_ok(rows, n)) != DA_OK) return rc;
  const int64_t per_row = ceil_div(n, RK_WAVE_KEYS), units = rows * per_row;
  const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(units, RK_THREADS / 64), 256 * 16);
  // the cache counts in 32 bits: a workgroup takes ceil(units / waves) units of 256 keys
  if (ceil_div(units, (int64_t)grid * (RK_THREADS / 64)) * RK_WAVE_KEYS * (RK_THREADS / 64) > 0xFFFFFFFFLL)
    return fail(DA_ERR_UNSUPPORTED, "key block too large for one launch");
  if (triangle)
    hipLaunchKernelGGL(k_rank_histogram<true>, dim3(grid), dim3(RK_THREADS), 0, stream, d_keys, n, ld, (uint32_t)nbins, d_hist, per_row, units,
                       row_begin, col_begin);
  else
    hipLaunchKernelGGL(k_rank_histogram<false>, dim3(grid), dim3(RK_THREADS), 0, stream, d_keys, n, ld, (uint32_t)nbins, d_hist, per_row, units,
                       row_begin, col_begin);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

}  // namespace da
