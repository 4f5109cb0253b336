// stats_kernels.hip -- the one thing compute_similarity_stats needs that a histogram cannot give: WHERE the extreme values of the strict
// upper triangle sit, under R's which(X == v, arr.ind = TRUE)[1, ] rule.
//
// k_upper_extrema: one pass over a block of keys -- `rows` rows of ld >= n keys, rows [row_begin, ...) x columns [col_begin, ...) of a square
// problem, the origin convention of k_rank_histogram -- that leaves one 20-byte record per row (da_row_extrema): over the elements whose
// global column is greater than the global row, the smallest and the largest rank with the FIRST local column holding each, and the rank
// of the row's diagonal element.  The reduction over the rows is host arithmetic on those records (api.cpp, stats_fold).
//   uint16 keys: MinHash counts (the key is its own rank) or NW codes ordered through the 65 536-entry table of da_nw_code_ranks;
//   uint32 keys: value ranks already (da_dev_nw_codes_to_ranks).
// The shape is k_threshold_count's: the workgroup owns a row (one wave when no row has more than 1024 masked keys), a thread
// takes 16 bytes per chunk where the row's address allows it and single keys otherwise, and what lies left of the diagonal is not read
// -- whole chunks by the loop's start, 16-byte units inside the first chunk by a test -- apart from the diagonal element itself.  A thread
// meets its columns in ascending order, so a strict compare keeps the first; between threads (rank, column) travel as one 64-bit word whose
// order is the rule -- min of rank << 32 | column, max of rank << 32 | ~column -- through shuffles, then LDS.  No atomics, no scratch.
#include "da_common.hpp"
#include "row_keys.hpp"

namespace da {
namespace {

constexpr int SX_THREADS = 256;
constexpr int SX_WAVE_SPAN = 1024;            // masked keys of a row up to which one wave owns it (k_threshold_count's rule)
constexpr uint32_t SX_NONE = 0xFFFFFFFFu;

__device__ __forceinline__ unsigned long long sx_min(unsigned long long a, unsigned long long b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned long long sx_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

template <typename Key, int THREADS>
__global__ __launch_bounds__(THREADS) void k_upper_extrema(const Key *__restrict__ keys, int64_t n, int64_t ld, const uint16_t *__restrict__ rank,
                                                           int64_t row_begin, int64_t col_begin, da_row_extrema *__restrict__ rec) {
  constexpr int PER = KeyRow<Key>::PER;
  constexpr int WAVES = THREADS / 64;
  constexpr int CHUNK = THREADS * PER;
  __shared__ unsigned long long wmin[WAVES], wmax[WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Key *row = keys + (int64_t)blockIdx.x * ld;
  const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  const int64_t diag = row_begin + (int64_t)blockIdx.x - col_begin;   // local column of the element on the global diagonal
  const int64_t first = diag + 1 > 0 ? diag + 1 : 0;                  // first masked local column: global column > global row
  uint32_t mn = SX_NONE, mn_c = SX_NONE, mx = 0, mx_c = SX_NONE;      // *_c == SX_NONE: nothing seen yet
  uint32_t r[PER], k[PER];
  for (int64_t c0 = first / CHUNK * CHUNK; c0 < n; c0 += CHUNK) {     // chunks left of the mask are not read
    const int64_t j0 = c0 + (int64_t)tid * PER;
    if (j0 + PER <= first) continue;                                  // nor the units of the first chunk that end before it
    const int nv = KeyRow<Key>::load(row, j0, n, vec, rank, r, k);
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      if (e >= nv || j0 + e < first) continue;
      const uint32_t v = r[e], c = (uint32_t)(j0 + e);
      if (v < mn || mn_c == SX_NONE) { mn = v; mn_c = c; }            // columns ascend within a thread: strict compares keep the first
      if (v > mx || mx_c == SX_NONE) { mx = v; mx_c = c; }
    }
  }
  // (rank, column) as one word: the smaller column wins a tie in both reductions; a thread that saw nothing is the neutral element of each
  unsigned long long kmin = ((unsigned long long)mn << 32) | mn_c;
  unsigned long long kmax = mx_c == SX_NONE ? 0ull : ((unsigned long long)mx << 32) | (uint32_t)~mx_c;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    kmin = sx_min(kmin, __shfl_down(kmin, o));
    kmax = sx_max(kmax, __shfl_down(kmax, o));
  }
  if (lane == 0) { wmin[wave] = kmin; wmax[wave] = kmax; }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < WAVES; ++w) { kmin = sx_min(kmin, wmin[w]); kmax = sx_max(kmax, wmax[w]); }
    da_row_extrema out;
    out.min_key = (uint32_t)(kmin >> 32);
    out.min_col = (int32_t)(uint32_t)kmin;                            // -1 when the row has no masked element
    out.max_key = (uint32_t)(kmax >> 32);
    out.max_col = (int32_t)~(uint32_t)kmax;                           // likewise
    out.diag_key = diag >= 0 && diag < n ? KeyRow<Key>::rank_of(row[diag], rank) : SX_NONE;
    rec[blockIdx.x] = out;
  }
}

template <typename Key>
int launch_extrema(const Key *d_keys, int64_t rows, int64_t n, int64_t ld, const uint16_t *d_rank, int64_t row_begin, int64_t col_begin,
                   da_row_extrema *d_rec, hipStream_t stream) {
  if (rows <= 0) return DA_OK;
  int rc;
  if ((rc = block_shape_ok(rows, n)) != DA_OK) return rc;
  // the longest masked span is the first row's
  const int64_t first0 = row_begin + 1 - col_begin, span = n - (first0 > 0 ? first0 : 0);
  if (span <= SX_WAVE_SPAN)
    hipLaunchKernelGGL((k_upper_extrema<Key, 64>), dim3((unsigned)rows), dim3(64), 0, stream, d_keys, n, ld, d_rank, row_begin, col_begin, d_rec);
  else
    hipLaunchKernelGGL((k_upper_extrema<Key, SX_THREADS>), dim3((unsigned)rows), dim3(SX_THREADS), 0, stream, d_keys, n, ld, d_rank, row_begin,
                       col_begin, d_rec);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

}  // namespace

int launch_upper_extrema(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, const uint16_t *d_rank, int64_t row_begin, int64_t col_begin,
                         da_row_extrema *d_rec, hipStream_t stream) {
  return launch_extrema(d_keys, rows, n, ld, d_rank, row_begin, col_begin, d_rec, stream);
}

int launch_upper_extrema32(const uint32_t *d_keys, int64_t rows, int64_t n, int64_t ld, int64_t row_begin, int64_t col_begin, da_row_extrema *d_rec,
                           hipStream_t stream) {
  return launch_extrema(d_keys, rows, n, ld, static_cast<const uint16_t *>(nullptr), row_begin, col_begin, d_rec, stream);
}

}  // namespace da
