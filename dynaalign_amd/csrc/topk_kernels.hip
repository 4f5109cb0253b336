// topk_kernels.hip -- the step after the two-set rectangle for a caller that keeps, per query, only its few most similar library entries:
// exact top-k per row of the uint16 count / code block the rectangle compare (da_dev_mh_compare_rect, da_dev_nw_rect) wrote, so that
// m x top numbers leave the device instead of the m x n matrix.
//
// Order: (rank descending, column ascending), rank = d_rank[key] or the key itself -- numpy's argsort(-rank, kind = "stable")[:top].  The
// rank table exists because equal VALUES must tie where their codes differ (NW 2/4 and 3/6, da_nw_code_ranks).
//
// One workgroup per row; the row is never sorted:
//   1. radix select on the rank, two 8-bit digits (the top 8 of rank_bits, then the rest): a 256-bin LDS histogram each, read from the top
//      by one wave -> T, the rank of the top-th element, and `above`, the number of elements above T;
//   2. ordered compaction: every element above T, and the first top - above elements equal to T in column order -- a workgroup prefix scan
//      per chunk of the row (wg_excl_scan, scan.hpp), so the choice among equals does not depend on scheduling;
//   3. the <= top candidates, as 64-bit words rank : ~column : key, sorted in LDS (wg_bitonic_sort, scan.hpp) and stored.
// The row is read three times (the second and third time from L2 / MALL); rank 0 -- by far the commonest: unrelated peptides share no
// k-mer -- is counted in a register, not with 64 lanes on one LDS word (k_upper_histogram does the same).
//
// k_topk_ranks is the same selection on uint32 keys that ARE value ranks (da_dev_nw_codes_to_ranks: NW sequences up to 1024 residues need 21
// bits): ceil(rank_bits / 8) digits instead of two, no table, candidates rank : ~column.  It is a sibling and not a Key parameter of
// k_topk_rows so that the uint16 kernels' code and registers stay exactly what DESIGN.md records.
#include "da_common.hpp"
#include "row_keys.hpp"

namespace da {
namespace {

// hist[0 .. 256) read from the top by wave 0: the bin B holding the want-th largest element (1-based) and the count in the bins above B
__device__ __forceinline__ void pick_bin(const unsigned int *hist, uint32_t want, unsigned int *out_bin, unsigned int *out_above) {
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x;
  uint32_t c[4], s = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) { c[q] = hist[255 - 4 * lane - q]; s += c[q]; }
  const uint32_t incl = wave_incl_scan(s);
  uint32_t acc = incl - s;
  if (acc < want && want <= incl) {            // exactly one lane when the histogram holds >= want elements
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (acc < want && want <= acc + c[q]) { *out_bin = (unsigned)(255 - 4 * lane - q); *out_above = acc; }
      acc += c[q];
    }
  }
}

// SELF: the block's row r owns column self_col0 + r (a row block of a square problem) and that element is absent from all three passes, so
// T, above, need_eq and the choice among equals are those of the row without it; its key goes to self_key[r] when that pointer is given (the
// NW diagonal).  An own column outside [0, n) excludes nothing.
template <int THREADS, bool SELF>
__global__ __launch_bounds__(THREADS) void k_topk_rows(const uint16_t *__restrict__ keys, int64_t n, int64_t ld,
                                                       const uint16_t *__restrict__ rank, int shift, int top, int32_t *__restrict__ idx,
                                                       int64_t ld_idx, uint16_t *__restrict__ key_out, int64_t ld_key, int64_t self_col0,
                                                       uint16_t *__restrict__ self_key) {
  constexpr int WAVES = THREADS / 64;
  constexpr int CHUNK = THREADS * TK_PER;
  __shared__ unsigned int hist[256];
  __shared__ unsigned long long cand[DA_TOPK_MAX];
  __shared__ unsigned int wtot[2][WAVES];
  __shared__ unsigned int sel[4];             // bin, above (high digit), bin, above (low digit)
  const int tid = threadIdx.x, lane = tid & 63;
  const uint16_t *row = keys + (int64_t)blockIdx.x * ld;
  const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  const uint32_t lo_mask = (1u << shift) - 1u;
  uint32_t r[TK_PER], k[TK_PER];
  const int64_t own = SELF ? self_col0 + (int64_t)blockIdx.x : -1;   // e == own - j0 names the own element inside a thread's TK_PER columns

  // ---- 1a. the high digit
  for (int b = tid; b < 256; b += THREADS) hist[b] = 0;
  if (tid < 4) sel[tid] = 0;
  __syncthreads();
  uint32_t zeros = 0;
  for (int64_t c0 = 0; c0 < n; c0 += CHUNK) {
    const int64_t j0 = c0 + (int64_t)tid * TK_PER;
    const int nv = KeyRow<uint16_t>::load(row, j0, n, vec, rank, r, k);
#pragma unroll
    for (int e = 0; e < TK_PER; ++e) {
      if (e >= nv) continue;
      if (SELF && own - j0 == e) {
        if (self_key) self_key[blockIdx.x] = (uint16_t)k[e];
        continue;
      }
      if (r[e] == 0) ++zeros;
      else { const uint32_t h = r[e] >> shift; atomicAdd(&hist[h < 255u ? h : 255u], 1u); }
    }
  }
  for (int o = 32; o > 0; o >>= 1) zeros += __shfl_down(zeros, o);
  if (lane == 0 && zeros) atomicAdd(&hist[0], zeros);
  __syncthreads();
  pick_bin(hist, (uint32_t)top, &sel[0], &sel[1]);
  __syncthreads();
  const uint32_t B = sel[0], above_hi = sel[1];
  uint32_t T = B, above = above_hi;
  // ---- 1b. the low digit among the elements of bin B
  if (shift > 0) {                             // block-uniform
    for (int b = tid; b < 256; b += THREADS) hist[b] = 0;
    __syncthreads();
    zeros = 0;
    for (int64_t c0 = 0; c0 < n; c0 += CHUNK) {
      const int64_t j0 = c0 + (int64_t)tid * TK_PER;
      const int nv = KeyRow<uint16_t>::load(row, j0, n, vec, rank, r, k);
#pragma unroll
      for (int e = 0; e < TK_PER; ++e) {
        if (e >= nv) continue;
        if (SELF && own - j0 == e) continue;
        if (r[e] == 0) { if (B == 0) ++zeros; }
        else if ((r[e] >> shift) == B) atomicAdd(&hist[r[e] & lo_mask], 1u);
      }
    }
    for (int o = 32; o > 0; o >>= 1) zeros += __shfl_down(zeros, o);
    if (lane == 0 && zeros) atomicAdd(&hist[0], zeros);
    __syncthreads();
    pick_bin(hist, (uint32_t)top - above_hi, &sel[2], &sel[3]);
    __syncthreads();
    T = (B << shift) | sel[2];
    above = above_hi + sel[3];
  }
  const uint32_t need_eq = (uint32_t)top - above;       // >= 1: the top-th element itself has rank T

  // ---- 2. ordered compaction.  Per chunk one scan of (elements above T) | (elements equal to T) << 16: <= 2048 each, no carry between them
  uint32_t gt_run = 0, eq_run = 0;
  int buf = 0;
  for (int64_t c0 = 0; c0 < n; c0 += CHUNK, buf ^= 1) {
    const int64_t j0 = c0 + (int64_t)tid * TK_PER;
    const int nv = KeyRow<uint16_t>::load(row, j0, n, vec, rank, r, k);
    uint32_t mine = 0;
#pragma unroll
    for (int e = 0; e < TK_PER; ++e)
      if (e < nv && !(SELF && own - j0 == e)) mine += r[e] > T ? 1u : (r[e] == T ? 0x10000u : 0u);
    uint32_t total;
    const uint32_t pre = wg_excl_scan<WAVES>(mine, wtot[buf], &total);   // the other buffer is written next time: one barrier per chunk
    uint32_t gt_at = gt_run + (pre & 0xFFFFu), eq_at = eq_run + (pre >> 16);
    if (mine) {
#pragma unroll
      for (int e = 0; e < TK_PER; ++e) {
        if (e >= nv || (SELF && own - j0 == e)) continue;
        const unsigned long long word = ((unsigned long long)r[e] << 48) | ((unsigned long long)(~(uint32_t)(j0 + e)) << 16) | k[e];
        if (r[e] > T) {
          if (gt_at < above && gt_at < (uint32_t)DA_TOPK_MAX) cand[gt_at] = word;
          ++gt_at;
        } else if (r[e] == T) {
          if (eq_at < need_eq && above + eq_at < (uint32_t)DA_TOPK_MAX) cand[above + eq_at] = word;
          ++eq_at;
        }
      }
    }
    gt_run += total & 0xFFFFu;
    eq_run += total >> 16;
  }

  // ---- 3. sort the candidates: descending words = rank descending, then ~column descending = column ascending
  int P = 1;
  while (P < top) P <<= 1;
  __syncthreads();
  for (int s = top + tid; s < P; s += THREADS) cand[s] = 0;     // below every candidate (~column is never 0)
  __syncthreads();
  wg_bitonic_sort<true, THREADS>(cand, P);
  for (int t = tid; t < top; t += THREADS) {
    const unsigned long long w = cand[t];
    idx[(int64_t)blockIdx.x * ld_idx + t] = (int32_t)(~(uint32_t)(w >> 16));
    key_out[(int64_t)blockIdx.x * ld_key + t] = (uint16_t)(w & 0xFFFFu);
  }
}

// The selection on uint32 value ranks: `digits` 8-bit digits (1 .. 4), most significant first; per digit only the elements whose higher
// digits equal the prefix found so far are counted.  A key above `rmax` (the largest value `digits` digits hold; keys are < nbins <= rmax + 1
// by contract) is taken as rmax: a wrong selection for a caller who breaks the contract, the same in every pass, never an access out of bounds.
// SELF as in k_topk_rows.  The candidate word is rank << 32 | ~column: the key IS the rank.
template <int THREADS, bool SELF>
__global__ __launch_bounds__(THREADS) void k_topk_ranks(const uint32_t *__restrict__ keys, int64_t n, int64_t ld, int digits, uint32_t rmax, int top,
                                                        int32_t *__restrict__ idx, int64_t ld_idx, uint32_t *__restrict__ key_out, int64_t ld_key,
                                                        int64_t self_col0, uint32_t *__restrict__ self_key) {
  constexpr int WAVES = THREADS / 64;
  constexpr int PER = KeyRow<uint32_t>::PER;
  constexpr int CHUNK = THREADS * PER;
  __shared__ unsigned int hist[256];
  __shared__ unsigned long long cand[DA_TOPK_MAX];
  __shared__ unsigned int wtot[2][WAVES];
  __shared__ unsigned int sel[2];             // bin, above of the digit at hand
  const int tid = threadIdx.x, lane = tid & 63;
  const uint32_t *row = keys + (int64_t)blockIdx.x * ld;
  const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  uint32_t r[PER];
  const int64_t own = SELF ? self_col0 + (int64_t)blockIdx.x : -1;   // e == own - j0 names the own element inside a thread's PER columns

  // ---- 1. the digits: T = the rank of the top-th element, above = the number of elements above T
  uint32_t T = 0, above = 0;                   // T: the digits found so far
  if (tid < 2) sel[tid] = 0;
  for (int d = digits - 1; d >= 0; --d) {      // block-uniform
    const int shift = 8 * d;
    for (int b = tid; b < 256; b += THREADS) hist[b] = 0;
    __syncthreads();
    uint32_t zeros = 0;
    for (int64_t c0 = 0; c0 < n; c0 += CHUNK) {
      const int64_t j0 = c0 + (int64_t)tid * PER;
      const int nv = KeyRow<uint32_t>::load(row, j0, n, vec, r);
#pragma unroll
      for (int e = 0; e < PER; ++e) {
        if (e >= nv) continue;
        if (SELF && own - j0 == e) {
          if (self_key && d == digits - 1) self_key[blockIdx.x] = r[e];
          continue;
        }
        const uint32_t v = r[e] < rmax ? r[e] : rmax, h = v >> shift;
        if (v == 0) { if (T == 0) ++zeros; }
        else if ((h >> 8) == T) atomicAdd(&hist[h & 255u], 1u);
      }
    }
    for (int o = 32; o > 0; o >>= 1) zeros += __shfl_down(zeros, o);
    if (lane == 0 && zeros) atomicAdd(&hist[0], zeros);
    __syncthreads();
    pick_bin(hist, (uint32_t)top - above, &sel[0], &sel[1]);
    __syncthreads();
    T = (T << 8) | sel[0];
    above += sel[1];
  }
  const uint32_t need_eq = (uint32_t)top - above;       // >= 1: the top-th element itself has rank T

  // ---- 2. ordered compaction.  Per chunk one scan of (elements above T) | (elements equal to T) << 16: <= 1024 each, no carry between them
  uint32_t gt_run = 0, eq_run = 0;
  int buf = 0;
  for (int64_t c0 = 0; c0 < n; c0 += CHUNK, buf ^= 1) {
    const int64_t j0 = c0 + (int64_t)tid * PER;
    const int nv = KeyRow<uint32_t>::load(row, j0, n, vec, r);
    uint32_t mine = 0;
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      r[e] = r[e] < rmax ? r[e] : rmax;
      if (e < nv && !(SELF && own - j0 == e)) mine += r[e] > T ? 1u : (r[e] == T ? 0x10000u : 0u);
    }
    uint32_t total;
    const uint32_t pre = wg_excl_scan<WAVES>(mine, wtot[buf], &total);   // the other buffer is written next time: one barrier per chunk
    uint32_t gt_at = gt_run + (pre & 0xFFFFu), eq_at = eq_run + (pre >> 16);
    if (mine) {
#pragma unroll
      for (int e = 0; e < PER; ++e) {
        if (e >= nv || (SELF && own - j0 == e)) continue;
        const unsigned long long word = ((unsigned long long)r[e] << 32) | (unsigned long long)(~(uint32_t)(j0 + e));
        if (r[e] > T) {
          if (gt_at < above && gt_at < (uint32_t)DA_TOPK_MAX) cand[gt_at] = word;
          ++gt_at;
        } else if (r[e] == T) {
          if (eq_at < need_eq && above + eq_at < (uint32_t)DA_TOPK_MAX) cand[above + eq_at] = word;
          ++eq_at;
        }
      }
    }
    gt_run += total & 0xFFFFu;
    eq_run += total >> 16;
  }

  // ---- 3. sort the candidates: descending words = rank descending, then ~column descending = column ascending
  int P = 1;
  while (P < top) P <<= 1;
  __syncthreads();
  for (int s = top + tid; s < P; s += THREADS) cand[s] = 0;     // below every candidate (~column is never 0)
  __syncthreads();
  wg_bitonic_sort<true, THREADS>(cand, P);
  for (int t = tid; t < top; t += THREADS) {
    const unsigned long long w = cand[t];
    idx[(int64_t)blockIdx.x * ld_idx + t] = (int32_t)(~(uint32_t)w);
    key_out[(int64_t)blockIdx.x * ld_key + t] = (uint32_t)(w >> 32);
  }
}

// the selected MinHash counts as similarities: the reference's divide (src/minHash.cpp:174)
__global__ __launch_bounds__(256) void k_topk_values(const uint16_t *__restrict__ key, int64_t ld_key, int64_t rows, int top, int n_hash,
                                                     double *__restrict__ val, int64_t ld_val) {
  const int64_t count = rows * top, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
    const int64_t rr = i / top, t = i - rr * top;
    val[rr * ld_val + t] = (double)key[rr * ld_key + t] / (double)n_hash;
  }
}

}  // namespace

namespace {
// what both selections check, rows > 0
int topk_launch_check(int64_t rows, int64_t n, int top, bool self) {
  if (self) {
    if (top < 1 || top > n - 1)
      return fail(DA_ERR_BAD_ARG, "top must be in 1 .. n - 1 when a row's own column is excluded (got top = %d, n = %lld)", top, (long long)n);
  } else if (top < 1 || top > n) return fail(DA_ERR_BAD_ARG, "top must be in 1 .. n (got top = %d, n = %lld)", top, (long long)n);
  if (top > DA_TOPK_MAX)
    return fail(DA_ERR_UNSUPPORTED, "top-k per row keeps its candidates in a fixed LDS buffer: top <= %d (got %d)", DA_TOPK_MAX, top);
  return block_shape_ok(rows, n);
}
int topk_rows_launch(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, const uint16_t *d_rank, int rank_bits, int top, int32_t *d_idx,
                     int64_t ld_idx, uint16_t *d_key_out, int64_t ld_key, bool self, int64_t self_col0, uint16_t *d_self_key, hipStream_t stream) {
  if (rows <= 0) return DA_OK;
  int rc;
  if ((rc = topk_launch_check(rows, n, top, self)) != DA_OK) return rc;
  if (rank_bits <= 0 || rank_bits > 16) rank_bits = 16;
  const int shift = rank_bits > 8 ? rank_bits - 8 : 0;
  // a row of up to 1024 keys is two chunks of one wave: four times as many rows in flight per CU as with 256 threads
  const bool wave = n <= 1024;
  auto kernel = wave ? (self ? k_topk_rows<64, true> : k_topk_rows<64, false>) : (self ? k_topk_rows<256, true> : k_topk_rows<256, false>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)rows), dim3(wave ? 64 : 256), 0, stream, d_keys, n, ld, d_rank, shift, top, d_idx, ld_idx, d_key_out, ld_key,
                     self_col0, d_self_key);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}
}  // namespace

int launch_topk_rows(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, const uint16_t *d_rank, int rank_bits, int top, int32_t *d_idx,
                     int64_t ld_idx, uint16_t *d_key_out, int64_t ld_key, hipStream_t stream) {
  return topk_rows_launch(d_keys, rows, n, ld, d_rank, rank_bits, top, d_idx, ld_idx, d_key_out, ld_key, false, 0, nullptr, stream);
}

int launch_topk_rows_self(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, const uint16_t *d_rank, int rank_bits, int top, int64_t self_col0,
                          int32_t *d_idx, int64_t ld_idx, uint16_t *d_key_out, int64_t ld_key, uint16_t *d_self_key, hipStream_t stream) {
  return topk_rows_launch(d_keys, rows, n, ld, d_rank, rank_bits, top, d_idx, ld_idx, d_key_out, ld_key, true, self_col0, d_self_key, stream);
}

namespace {
int topk_ranks_launch(const uint32_t *d_keys, int64_t rows, int64_t n, int64_t ld, int64_t nbins, int top, int32_t *d_idx, int64_t ld_idx,
                      uint32_t *d_key_out, int64_t ld_key, bool self, int64_t self_col0, uint32_t *d_self_key, hipStream_t stream) {
  if (rows <= 0) return DA_OK;
  int rc;
  if ((rc = topk_launch_check(rows, n, top, self)) != DA_OK) return rc;
  if (nbins < 1 || nbins > 0x7fffffffLL) return fail(DA_ERR_BAD_ARG, "nbins must be in 1 .. 2^31 - 1 (got %lld)", (long long)nbins);
  int rank_bits = 1;                           // bits of nbins - 1, at least one
  while (rank_bits < 31 && ((nbins - 1) >> rank_bits) != 0) ++rank_bits;
  const int digits = (rank_bits + 7) / 8;
  const uint32_t rmax = digits == 4 ? 0xFFFFFFFFu : (1u << (8 * digits)) - 1u;
  // a row of up to 1024 keys is four chunks of one wave: four times as many rows in flight per CU as with 256 threads
  const bool wave = n <= 1024;
  auto kernel = wave ? (self ? k_topk_ranks<64, true> : k_topk_ranks<64, false>) : (self ? k_topk_ranks<256, true> : k_topk_ranks<256, false>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)rows), dim3(wave ? 64 : 256), 0, stream, d_keys, n, ld, digits, rmax, top, d_idx, ld_idx, d_key_out, ld_key,
                     self_col0, d_self_key);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}
}  // namespace

int launch_topk_ranks(const uint32_t *d_keys, int64_t rows, int64_t n, int64_t ld, int64_t nbins, int top, int32_t *d_idx, int64_t ld_idx,
                      uint32_t *d_key_out, int64_t ld_key, hipStream_t stream) {
  return topk_ranks_launch(d_keys, rows, n, ld, nbins, top, d_idx, ld_idx, d_key_out, ld_key, false, 0, nullptr, stream);
}

int launch_topk_ranks_self(const uint32_t *d_keys, int64_t rows, int64_t n, int64_t ld, int64_t nbins, int top, int64_t self_col0, int32_t *d_idx,
                           int64_t ld_idx, uint32_t *d_key_out, int64_t ld_key, uint32_t *d_self_key, hipStream_t stream) {
  return topk_ranks_launch(d_keys, rows, n, ld, nbins, top, d_idx, ld_idx, d_key_out, ld_key, true, self_col0, d_self_key, stream);
}

int launch_topk_values(const uint16_t *d_key, int64_t ld_key, int64_t rows, int top, int n_hash, double *d_val, int64_t ld_val, hipStream_t stream) {
  if (rows <= 0 || top <= 0) return DA_OK;
  int64_t blocks = ceil_div(rows * top, 256);
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(k_topk_values, dim3((unsigned)blocks), dim3(256), 0, stream, d_key, ld_key, rows, top, n_hash, d_val, ld_val);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

}  // namespace da
