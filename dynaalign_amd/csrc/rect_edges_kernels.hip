// rect_edges_kernels.hip -- the threshold form of the two-set rectangle: of the uint16 count / code block the rectangle compare
// (da_dev_mh_compare_rect, da_dev_nw_rect) wrote, only the entries whose value passes a threshold leave the device, as rows of
// (column, key) in ascending column order -- a CSR block -- instead of the m x n matrix.
//
// Unlike the square path (graph_kernels.hip: tiles of the triangle appended in arrival order through one global counter, sorted on the
// host) a rectangle has independent rows and nothing to skip, so the list is produced in its final order:
//   1. k_rect_histogram (quantile form only): the histogram of the whole block, for the host's type-7 quantile;
//   2. k_threshold_count: per row, the number of keys flagged in keep[]; an exclusive scan of those (hipcub) gives the row pointers;
//   3. k_threshold_emit: ordered compaction.  The workgroup that owns a row walks it in chunks, scans the per-thread kept counts of a chunk,
//      carries a running base from chunk to chunk, and every thread writes its own contiguous run of slots.  No output atomic, no sort: the
//      slot of an entry depends on the data alone.
// Rows of up to 1024 keys take one wave each (k_topk_rows' rule): four times as many rows in flight per CU as with 256 threads.  Key 0 -- by
// far the commonest: unrelated peptides share no k-mer -- is decided from a register, not through the keep table.
#include "da_common.hpp"

#include <algorithm>

#include <hipcub/hipcub.hpp>

namespace da {
namespace {

constexpr int RE_THREADS = 256;
constexpr int RE_LDS_BINS = 8192;             // 32 KiB, as k_upper_histogram: MinHash counts and NW codes of short peptides stay in LDS
constexpr int RE_WAVE_KEYS = 64 * TK_PER;     // what one wave takes per step of the histogram

inline size_t up256(size_t b) { return (b + 255) / 256 * 256; }

// hist[v] += number of keys equal to v in the block.  Persistent workgroups (the LDS histogram is cleared and flushed once per workgroup); the
// unit of work is 512 consecutive keys of one row per WAVE, so that a block of many short rows keeps every wave busy.
__global__ __launch_bounds__(RE_THREADS) void k_rect_histogram(const uint16_t *__restrict__ keys, int64_t n, int64_t ld, int nbins,
                                                               unsigned long long *__restrict__ hist, int64_t per_row, int64_t units) {
  __shared__ unsigned int lh[RE_LDS_BINS];
  const bool use_lds = nbins <= RE_LDS_BINS;
  if (use_lds)
    for (int b = threadIdx.x; b < nbins; b += RE_THREADS) lh[b] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (RE_THREADS / 64);
  unsigned long long zeros = 0;               // same-address LDS atomics of 64 lanes serialise: the common value stays in a register
  uint32_t r[TK_PER], k[TK_PER];
  for (int64_t u = (int64_t)blockIdx.x * (RE_THREADS / 64) + (threadIdx.x >> 6); u < units; u += nwaves) {
    const int64_t rr = u / per_row, c = u - rr * per_row;
    const uint16_t *row = keys + rr * ld;
    const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    const int nv = load8(row, c * RE_WAVE_KEYS + (int64_t)lane * TK_PER, n, vec, nullptr, r, k);
    unsigned z = 0;
#pragma unroll
    for (int e = 0; e < TK_PER; ++e) {
      if (e >= nv) continue;
      const uint32_t v = k[e];
      if (v == 0) ++z;
      else if (v < (uint32_t)nbins) {
        if (use_lds) atomicAdd(&lh[v], 1u);
        else atomicAdd(&hist[v], 1ull);
      }
    }
    zeros += z;
  }
  for (int o = 32; o > 0; o >>= 1) zeros += __shfl_down(zeros, o);
  if (lane == 0 && zeros) atomicAdd(&hist[0], zeros);
  __syncthreads();
  if (use_lds)
    for (int b = threadIdx.x; b < nbins; b += RE_THREADS)
      if (lh[b]) atomicAdd(&hist[b], (unsigned long long)lh[b]);
}

// bit e set: column j0 + e exists and its key is flagged
__device__ __forceinline__ uint32_t kept_mask(const uint32_t k[TK_PER], int nv, const uint8_t *__restrict__ keep, uint32_t nbins, bool keep0) {
  uint32_t mask = 0;
#pragma unroll
  for (int e = 0; e < TK_PER; ++e) {
    if (e >= nv) continue;
    const uint32_t v = k[e];
    const bool kp = v == 0 ? keep0 : (v < nbins && keep[v] != 0);
    mask |= (kp ? 1u : 0u) << e;
  }
  return mask;
}

// cnt[row] = number of flagged keys of the row; one workgroup (THREADS = 64: one wave) per row
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_threshold_count(const uint16_t *__restrict__ keys, int64_t n, int64_t ld,
                                                             const uint8_t *__restrict__ keep, int nbins, long long *__restrict__ cnt) {
  constexpr int WAVES = THREADS / 64;
  constexpr int CHUNK = THREADS * TK_PER;
  __shared__ unsigned int wsum[WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint16_t *row = keys + (int64_t)blockIdx.x * ld;
  const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  const bool keep0 = keep[0] != 0;
  uint32_t r[TK_PER], k[TK_PER], mine = 0;
  for (int64_t c0 = 0; c0 < n; c0 += CHUNK) {
    const int nv = load8(row, c0 + (int64_t)tid * TK_PER, n, vec, nullptr, r, k);
    mine += (uint32_t)__popc(kept_mask(k, nv, keep, (uint32_t)nbins, keep0));
  }
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o);
  if (lane == 0) wsum[wave] = mine;
  __syncthreads();
  if (tid == 0) {
    long long total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) total += wsum[w];
    cnt[blockIdx.x] = total;
  }
}

// the flagged columns of the row, ascending, at slots rowptr[row] ...; slots >= capacity are not written
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_threshold_emit(const uint16_t *__restrict__ keys, int64_t n, int64_t ld,
                                                            const uint8_t *__restrict__ keep, int nbins, const long long *__restrict__ rowptr,
                                                            int32_t *__restrict__ out_j, uint16_t *__restrict__ out_key, long long capacity) {
  constexpr int WAVES = THREADS / 64;
  constexpr int CHUNK = THREADS * TK_PER;
  __shared__ unsigned int wtot[2][WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long base = rowptr[blockIdx.x];
  if (rowptr[blockIdx.x + 1] == base || base >= capacity) return;   // block-uniform: a row without an edge is not read again
  const uint16_t *row = keys + (int64_t)blockIdx.x * ld;
  const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  const bool keep0 = keep[0] != 0;
  uint32_t r[TK_PER], k[TK_PER];
  int buf = 0;
  for (int64_t c0 = 0; c0 < n; c0 += CHUNK, buf ^= 1) {
    const int64_t j0 = c0 + (int64_t)tid * TK_PER;
    const int nv = load8(row, j0, n, vec, nullptr, r, k);
    const uint32_t mask = kept_mask(k, nv, keep, (uint32_t)nbins, keep0);
    const uint32_t mine = (uint32_t)__popc(mask);
    const uint32_t incl = wave_incl_scan(mine);
    if (lane == 63) wtot[buf][wave] = incl;
    __syncthreads();                           // the other buffer is written next time: one barrier per chunk
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      const uint32_t t = wtot[buf][w];
      if (w < wave) before += t;
      total += t;
    }
    if (mine) {
      long long slot = base + before + incl - mine;
#pragma unroll
      for (int e = 0; e < TK_PER; ++e) {
        if (!(mask & (1u << e))) continue;
        if (slot < capacity) {
          out_j[slot] = (int32_t)(j0 + e);
          out_key[slot] = (uint16_t)k[e];
        }
        ++slot;
      }
    }
    base += total;
  }
}

// the kept MinHash counts as similarities: the reference's divide (src/minHash.cpp:174), as k_topk_values
__global__ __launch_bounds__(256) void k_edge_values(const uint16_t *__restrict__ key, int64_t count, int n_hash, double *__restrict__ w) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) w[i] = (double)key[i] / (double)n_hash;
}

__global__ __launch_bounds__(256) void k_rowptr_offset(const long long *__restrict__ in, int64_t count, long long base, long long *__restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) out[i] = in[i] + base;
}

int block_shape_ok(int64_t rows, int64_t n) {
  if (rows > 0x7fffffffLL || n > 0x7ffffff0LL) return fail(DA_ERR_UNSUPPORTED, "key block too large for one launch");
  return DA_OK;
}

}  // namespace

int launch_rect_histogram(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, int nbins, unsigned long long *d_hist, hipStream_t stream) {
  if (rows <= 0 || n <= 0) return DA_OK;
  int rc;
  if ((rc = block_shape_ok(rows, n)) != DA_OK) return rc;
  const int64_t per_row = ceil_div(n, RE_WAVE_KEYS), units = rows * per_row;
  const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(units, RE_THREADS / 64), 256 * 16);
  hipLaunchKernelGGL(k_rect_histogram, dim3(grid), dim3(RE_THREADS), 0, stream, d_keys, n, ld, nbins, d_hist, per_row, units);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

// workspace: the per-row counts (rows + 1 int64, the last one 0) + the scan's own scratch
size_t threshold_rows_workspace_bytes(int64_t rows) {
  if (rows <= 0) return 256;
  size_t temp = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, temp, (const long long *)nullptr, (long long *)nullptr, (int)(rows + 1), nullptr);
  return up256((size_t)(rows + 1) * 8) + up256(temp) + 256;
}

// d_rowptr = exclusive scan of the rows + 1 per-row counts at the head of the workspace (the last one 0); the scan's scratch follows them
int threshold_rows_scan(void *d_work, size_t work_bytes, int64_t rows, int64_t *d_rowptr, hipStream_t stream) {
  long long *cnt = static_cast<long long *>(d_work);
  char *w = static_cast<char *>(d_work) + up256((size_t)(rows + 1) * 8);
  size_t temp = work_bytes - up256((size_t)(rows + 1) * 8);
  DA_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(w, temp, cnt, reinterpret_cast<long long *>(d_rowptr), (int)(rows + 1), stream));
  return DA_OK;
}

int launch_threshold_rows_count(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, const uint8_t *d_keep, int nbins, int64_t *d_rowptr,
                                void *d_work, size_t work_bytes, hipStream_t stream) {
  if (rows <= 0) return DA_OK;
  int rc;
  if ((rc = block_shape_ok(rows, n)) != DA_OK) return rc;
  if (n <= 0) { DA_HIP_TRY(hipMemsetAsync(d_rowptr, 0, (size_t)(rows + 1) * 8, stream)); return DA_OK; }
  if (rows + 1 > 0x7fffffffLL) return fail(DA_ERR_UNSUPPORTED, "key block too large for one launch");
  if (!d_work || work_bytes < threshold_rows_workspace_bytes(rows)) return fail(DA_ERR_BAD_ARG, "threshold rows: workspace too small");
  long long *cnt = static_cast<long long *>(d_work);
  DA_HIP_TRY(hipMemsetAsync(cnt + rows, 0, 8, stream));
  if (n <= 1024)
    hipLaunchKernelGGL(k_threshold_count<64>, dim3((unsigned)rows), dim3(64), 0, stream, d_keys, n, ld, d_keep, nbins, cnt);
  else
    hipLaunchKernelGGL(k_threshold_count<RE_THREADS>, dim3((unsigned)rows), dim3(RE_THREADS), 0, stream, d_keys, n, ld, d_keep, nbins, cnt);
  DA_HIP_TRY(hipGetLastError());
  return threshold_rows_scan(d_work, work_bytes, rows, d_rowptr, stream);
}

int launch_threshold_rows_emit(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, const uint8_t *d_keep, int nbins, const int64_t *d_rowptr,
                               int32_t *d_j, uint16_t *d_key_out, int64_t capacity, hipStream_t stream) {
  if (rows <= 0 || n <= 0 || capacity <= 0) return DA_OK;
  int rc;
  if ((rc = block_shape_ok(rows, n)) != DA_OK) return rc;
  const long long *rp = reinterpret_cast<const long long *>(d_rowptr);
  if (n <= 1024)
    hipLaunchKernelGGL(k_threshold_emit<64>, dim3((unsigned)rows), dim3(64), 0, stream, d_keys, n, ld, d_keep, nbins, rp, d_j, d_key_out,
                       (long long)capacity);
  else
    hipLaunchKernelGGL(k_threshold_emit<RE_THREADS>, dim3((unsigned)rows), dim3(RE_THREADS), 0, stream, d_keys, n, ld, d_keep, nbins, rp, d_j,
                       d_key_out, (long long)capacity);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

int launch_edge_values(const uint16_t *d_key, int64_t count, int n_hash, double *d_w, hipStream_t stream) {
  if (count <= 0) return DA_OK;
  const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(count, 256), 256 * 16);
  hipLaunchKernelGGL(k_edge_values, dim3(grid), dim3(256), 0, stream, d_key, count, n_hash, d_w);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

int launch_rowptr_offset(const int64_t *d_in, int64_t count, int64_t base, int64_t *d_out, hipStream_t stream) {
  if (count <= 0) return DA_OK;
  const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(count, 256), 256 * 16);
  hipLaunchKernelGGL(k_rowptr_offset, dim3(grid), dim3(256), 0, stream, reinterpret_cast<const long long *>(d_in), count, (long long)base,
                     reinterpret_cast<long long *>(d_out));
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

}  // namespace da
