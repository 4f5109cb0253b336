// rect_edges_kernels.hip -- the threshold form of the two-set rectangle: of the uint16 count / code block the rectangle compare
// (da_dev_mh_compare_rect, da_dev_nw_rect) wrote, only the entries whose value passes a threshold leave the device, as rows of
// (column, key) in ascending column order -- a CSR block -- instead of the m x n matrix.
//
// Unlike the square path (graph_kernels.hip: tiles of the triangle appended in arrival order through one global counter, sorted on the
// host) a rectangle has independent rows and nothing to skip, so the list is produced in its final order:
//   1. k_rect_histogram (quantile form only): the histogram of the whole block, for the host's type-7 quantile;
//   2. k_threshold_count: per row, the number of kept keys; an exclusive scan of those (hipcub) gives the row pointers;
//   3. k_threshold_emit: ordered compaction.  The workgroup that owns a row walks it in chunks, scans the per-thread kept counts of a chunk (wg_excl_scan, scan.hpp),
//      carries a running base from chunk to chunk, and every thread writes its own contiguous run of slots.  No output atomic, no sort: the
//      slot of an entry depends on the data alone.
// Rows of up to 1024 keys take one wave each (k_topk_rows' rule): four times as many rows in flight per CU as with 256 threads.
//
// Count and emit are templates over the key type (KeyRow<Key>, row_keys.hpp: 8 x uint16 or 4 x uint32 per 16-byte load) and a keep policy:
//   KeepTable  uint16 counts / codes flagged in keep[]; key 0 -- by far the commonest: unrelated peptides share no k-mer -- is decided from a
//              register, not through the table;
//   KeepRanks  uint32 value ranks >= r_min inside a rectangle or triangle mask (the NW edge list of long sequences, whose codes-to-ranks and
//              histogram steps are in nw_edges_long_kernels.hip).
#include "da_common.hpp"
#include "row_keys.hpp"

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
  uint32_t k[TK_PER];
  for (int64_t u = (int64_t)blockIdx.x * (RE_THREADS / 64) + (threadIdx.x >> 6); u < units; u += nwaves) {
    const int64_t rr = u / per_row, c = u - rr * per_row;
    const uint16_t *row = keys + rr * ld;
    const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    const int nv = KeyRow<uint16_t>::load(row, c * RE_WAVE_KEYS + (int64_t)lane * TK_PER, n, vec, k);
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

// ---- the keep decision of k_threshold_count / k_threshold_emit: a by-value policy.  first(row): the first local column of the row's mask;
// mask(k, nv, j0, first): bit e set when column j0 + e exists, lies in the mask and its key is kept; init(): what is read once per workgroup.
// uint16 keys flagged in a table; the mask is the whole row, so first() is a compile-time 0 and the column tests fold away
struct KeepTable {
  const uint8_t *__restrict__ keep;
  uint32_t nbins;
  bool keep0;                                  // keep[0], held in a register
  __device__ __forceinline__ void init() { keep0 = keep[0] != 0; }
  __device__ static __forceinline__ constexpr int64_t first(int64_t) { return 0; }
  __device__ __forceinline__ uint32_t mask(const uint32_t k[KeyRow<uint16_t>::PER], int nv, int64_t, int64_t) const {
    uint32_t m = 0;
#pragma unroll
    for (int e = 0; e < KeyRow<uint16_t>::PER; ++e) {
      if (e >= nv) continue;
      const uint32_t v = k[e];
      const bool kp = v == 0 ? keep0 : (v < nbins && keep[v] != 0);
      m |= (kp ? 1u : 0u) << e;
    }
    return m;
  }
};
// uint32 value ranks >= r_min; the mask is the rectangle or, tri, the upper triangle INCLUDING the diagonal of a square problem of which the
// block is rows [row_begin, ...) x columns [col_begin, ...): global column >= global row
struct KeepRanks {
  uint32_t r_min, nbins;
  int tri;
  int64_t row_begin, col_begin;
  __device__ __forceinline__ void init() {}
  __device__ __forceinline__ int64_t first(int64_t row) const {
    const int64_t f = tri ? row_begin + row - col_begin : 0;
    return f > 0 ? f : 0;
  }
  __device__ __forceinline__ uint32_t mask(const uint32_t k[KeyRow<uint32_t>::PER], int nv, int64_t j0, int64_t first) const {
    uint32_t m = 0;
#pragma unroll
    for (int e = 0; e < KeyRow<uint32_t>::PER; ++e) {
      const bool kp = e < nv && j0 + e >= first && k[e] >= r_min && k[e] < nbins;
      m |= (kp ? 1u : 0u) << e;
    }
    return m;
  }
};

// cnt[row] = number of kept keys of the row; one workgroup (THREADS = 64: one wave) per row
template <typename Key, typename Keep, int THREADS>
__global__ __launch_bounds__(THREADS) void k_threshold_count(const Key *__restrict__ keys, int64_t n, int64_t ld, Keep keep,
                                                             long long *__restrict__ cnt) {
  constexpr int PER = KeyRow<Key>::PER;
  constexpr int WAVES = THREADS / 64;
  constexpr int CHUNK = THREADS * PER;
  __shared__ unsigned int wsum[WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Key *row = keys + (int64_t)blockIdx.x * ld;
  const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  const int64_t first = keep.first(blockIdx.x);
  keep.init();
  uint32_t k[PER], mine = 0;
  for (int64_t c0 = first / CHUNK * CHUNK; c0 < n; c0 += CHUNK) {   // chunks left of the mask are not read
    const int64_t j0 = c0 + (int64_t)tid * PER;
    const int nv = KeyRow<Key>::load(row, j0, n, vec, k);
    mine += (uint32_t)__popc(keep.mask(k, nv, j0, first));
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

// the kept columns of the row (local to the block), ascending, at slots rowptr[row] ...; slots >= capacity are not written
template <typename Key, typename Keep, int THREADS>
__global__ __launch_bounds__(THREADS) void k_threshold_emit(const Key *__restrict__ keys, int64_t n, int64_t ld, Keep keep,
                                                            const long long *__restrict__ rowptr, int32_t *__restrict__ out_j,
                                                            Key *__restrict__ out_key, long long capacity) {
  constexpr int PER = KeyRow<Key>::PER;
  constexpr int WAVES = THREADS / 64;
  constexpr int CHUNK = THREADS * PER;
  __shared__ unsigned int wtot[2][WAVES];
  const int tid = threadIdx.x;
  long long base = rowptr[blockIdx.x];
  if (rowptr[blockIdx.x + 1] == base || base >= capacity) return;   // block-uniform: a row without an edge is not read again
  const Key *row = keys + (int64_t)blockIdx.x * ld;
  const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  const int64_t first = keep.first(blockIdx.x);
  keep.init();
  uint32_t k[PER];
  int buf = 0;
  for (int64_t c0 = first / CHUNK * CHUNK; c0 < n; c0 += CHUNK, buf ^= 1) {
    const int64_t j0 = c0 + (int64_t)tid * PER;
    const int nv = KeyRow<Key>::load(row, j0, n, vec, k);
    const uint32_t mask = keep.mask(k, nv, j0, first);
    const uint32_t mine = (uint32_t)__popc(mask);
    uint32_t total;
    const uint32_t pre = wg_excl_scan<WAVES>(mine, wtot[buf], &total);   // the other buffer is written next time: one barrier per chunk
    if (mine) {
      long long slot = base + pre;
#pragma unroll
      for (int e = 0; e < PER; ++e) {
        if (!(mask & (1u << e))) continue;
        if (slot < capacity) {
          out_j[slot] = (int32_t)(j0 + e);
          out_key[slot] = (Key)k[e];
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

// one launch of a workgroup-per-row kernel: a row of up to 1024 keys takes one wave, 256 threads beyond
template <typename K64, typename K256, typename... Args>
int launch_per_row(K64 k64, K256 k256, int64_t rows, int64_t n, hipStream_t stream, Args... args) {
  if (n <= 1024) hipLaunchKernelGGL(k64, dim3((unsigned)rows), dim3(64), 0, stream, args...);
  else hipLaunchKernelGGL(k256, dim3((unsigned)rows), dim3(RE_THREADS), 0, stream, args...);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

// the per-row counts (rows + 1 int64) into the head of the workspace, then their scan; `who` names the entry point in the workspace message
template <typename Key, typename Keep>
int threshold_count(const Key *d_keys, int64_t rows, int64_t n, int64_t ld, const Keep &keep, int64_t *d_rowptr, void *d_work, size_t work_bytes,
                    const char *who, hipStream_t stream) {
  if (rows <= 0) return DA_OK;
  int rc;
  if ((rc = block_shape_ok(rows, n)) != DA_OK) return rc;
  if (n <= 0) { DA_HIP_TRY(hipMemsetAsync(d_rowptr, 0, (size_t)(rows + 1) * 8, stream)); return DA_OK; }
  if (rows + 1 > 0x7fffffffLL) return fail(DA_ERR_UNSUPPORTED, "key block too large for one launch");
  if (!d_work || work_bytes < threshold_rows_workspace_bytes(rows)) return fail(DA_ERR_BAD_ARG, "%s: workspace too small", who);
  long long *cnt = static_cast<long long *>(d_work);
  DA_HIP_TRY(hipMemsetAsync(cnt + rows, 0, 8, stream));
  if ((rc = launch_per_row(k_threshold_count<Key, Keep, 64>, k_threshold_count<Key, Keep, RE_THREADS>, rows, n, stream, d_keys, n, ld, keep, cnt)) != DA_OK)
    return rc;
  // d_rowptr = exclusive scan of the rows + 1 counts (the last one 0); the scan's scratch follows them in the workspace
  const size_t head = up256((size_t)(rows + 1) * 8);
  size_t temp = work_bytes - head;
  DA_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(static_cast<char *>(d_work) + head, temp, cnt, reinterpret_cast<long long *>(d_rowptr), (int)(rows + 1), stream));
  return DA_OK;
}

template <typename Key, typename Keep>
int threshold_emit(const Key *d_keys, int64_t rows, int64_t n, int64_t ld, const Keep &keep, const int64_t *d_rowptr, int32_t *d_j, Key *d_key_out,
                   int64_t capacity, hipStream_t stream) {
  if (rows <= 0 || n <= 0 || capacity <= 0) return DA_OK;
  int rc;
  if ((rc = block_shape_ok(rows, n)) != DA_OK) return rc;
  return launch_per_row(k_threshold_emit<Key, Keep, 64>, k_threshold_emit<Key, Keep, RE_THREADS>, rows, n, stream, d_keys, n, ld, keep,
                        reinterpret_cast<const long long *>(d_rowptr), d_j, d_key_out, (long long)capacity);
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

int launch_threshold_rows_count(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, const uint8_t *d_keep, int nbins, int64_t *d_rowptr,
                                void *d_work, size_t work_bytes, hipStream_t stream) {
  return threshold_count(d_keys, rows, n, ld, KeepTable{d_keep, (uint32_t)nbins, false}, d_rowptr, d_work, work_bytes, "threshold rows", stream);
}

int launch_threshold_rows_emit(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, const uint8_t *d_keep, int nbins, const int64_t *d_rowptr,
                               int32_t *d_j, uint16_t *d_key_out, int64_t capacity, hipStream_t stream) {
  return threshold_emit(d_keys, rows, n, ld, KeepTable{d_keep, (uint32_t)nbins, false}, d_rowptr, d_j, d_key_out, capacity, stream);
}

int launch_threshold_ranks_count(const uint32_t *d_keys, int64_t rows, int64_t n, int64_t ld, uint32_t r_min, int64_t nbins, bool triangle,
                                 int64_t row_begin, int64_t col_begin, int64_t *d_rowptr, void *d_work, size_t work_bytes, hipStream_t stream) {
  return threshold_count(d_keys, rows, n, ld, KeepRanks{r_min, (uint32_t)nbins, triangle ? 1 : 0, row_begin, col_begin}, d_rowptr, d_work, work_bytes,
                         "threshold ranks", stream);
}

int launch_threshold_ranks_emit(const uint32_t *d_keys, int64_t rows, int64_t n, int64_t ld, uint32_t r_min, int64_t nbins, bool triangle,
                                int64_t row_begin, int64_t col_begin, const int64_t *d_rowptr, int32_t *d_j, uint32_t *d_key_out, int64_t capacity,
                                hipStream_t stream) {
  return threshold_emit(d_keys, rows, n, ld, KeepRanks{r_min, (uint32_t)nbins, triangle ? 1 : 0, row_begin, col_begin}, d_rowptr, d_j, d_key_out, capacity,
                        stream);
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
