// scan.hpp -- the prefix sums and the LDS sort every kernel file shares (internal linkage, like row_keys.hpp and lsh_common.hpp):
//   wave_incl_scan       inclusive scan over the 64 lanes of a wave, by shuffles;
//   wg_excl_scan         exclusive scan over a workgroup of WAVES waves, one barrier;
//   wave_scan_1024       exclusive scan, in place, of 1024 LDS counters by the workgroup's first wave;
//   launch_scan          exclusive scan of an array in global memory: one workgroup walking it (k_scan_block), or block sums, their scan by one
//                        workgroup and every block's own scan plus its offset (k_scan_sums, k_scan_block, k_scan_apply: three short launches);
//   wg_bitonic_sort      a power-of-two LDS array sorted by the workgroup.
// All sums are integers: the order of the additions does not show in the result.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace da {

// lanes up to and including `lane` summed
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  return v;
}

// The sum of v over the threads below this one; *total = the sum over the workgroup.  wsum: WAVES words of LDS that no thread may write again
// before every thread has returned -- a caller in a loop hands in two buffers in turn (then this barrier is the only one per round) or
// puts a barrier of its own behind the call.
template <int WAVES, typename T>
__device__ __forceinline__ T wg_excl_scan(T v, T *wsum, T *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T incl = wave_incl_scan(v);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  T before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const T t = wsum[w];
    if (w < wave) before += t;
    all += t;
  }
  *total = all;
  return before + incl - v;
}

// part[0 .. 1024) -> its exclusive prefix sums, by the first wave (16 counters per lane); the caller's barriers stand before and behind
__device__ __forceinline__ void wave_scan_1024(uint32_t *part) {
  if (threadIdx.x >= 64) return;
  uint32_t v[16], tot = 0;
#pragma unroll
  for (int q = 0; q < 16; ++q) { v[q] = part[threadIdx.x * 16 + q]; tot += v[q]; }
  uint32_t run = wave_incl_scan(tot) - tot;
#pragma unroll
  for (int q = 0; q < 16; ++q) { part[threadIdx.x * 16 + q] = run; run += v[q]; }
}

// ---- the grid scan.  Op (by value): load(i) -> uint64_t, element i < count as the word that is summed (two 32-bit sums may ride in its halves:
// two arrays for the cost of one scan); store(i, e): e = the sum of the elements before i; store_total(count, t): t = the sum of all.
constexpr int SCAN_BLOCK = 1024;

namespace {

template <typename Op>
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_block(Op op, int32_t count) {   // one workgroup
  __shared__ uint64_t wsum[2][SCAN_BLOCK / 64];
  uint64_t carry = 0;
  int buf = 0;
  for (int32_t base = 0; base < count; base += SCAN_BLOCK, buf ^= 1) {
    const int32_t i = base + (int32_t)threadIdx.x;
    uint64_t total;
    const uint64_t e = carry + wg_excl_scan<SCAN_BLOCK / 64>(i < count ? op.load(i) : (uint64_t)0, wsum[buf], &total);
    if (i < count) op.store(i, e);
    carry += total;
  }
  if (threadIdx.x == 0) op.store_total(count, carry);
}
struct ScanInPlace {   // the block sums of the wide form, scanned by k_scan_block: bsum[0 .. count] <- their exclusive scan and the total
  uint64_t *bsum;
  __device__ __forceinline__ uint64_t load(int32_t i) const { return bsum[i]; }
  __device__ __forceinline__ void store(int32_t i, uint64_t e) const { bsum[i] = e; }
  __device__ __forceinline__ void store_total(int32_t count, uint64_t t) const { bsum[count] = t; }
};

template <typename Op>
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_sums(Op op, int32_t count, uint64_t *__restrict__ bsum) {
  __shared__ uint64_t wsum[SCAN_BLOCK / 64];
  const int32_t i = blockIdx.x * SCAN_BLOCK + threadIdx.x;
  uint64_t x = i < count ? op.load(i) : (uint64_t)0;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = x;
  __syncthreads();
  if (threadIdx.x == 0) { uint64_t t = 0; for (int w = 0; w < SCAN_BLOCK / 64; ++w) t += wsum[w]; bsum[blockIdx.x] = t; }
}
template <typename Op>
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_apply(Op op, int32_t count, const uint64_t *__restrict__ bsum) {
  __shared__ uint64_t wsum[SCAN_BLOCK / 64];
  const int32_t i = blockIdx.x * SCAN_BLOCK + threadIdx.x;
  uint64_t total;
  const uint64_t e = bsum[blockIdx.x] + wg_excl_scan<SCAN_BLOCK / 64>(i < count ? op.load(i) : (uint64_t)0, wsum, &total);
  if (i < count) op.store(i, e);
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) op.store_total(count, bsum[gridDim.x]);
}

// count >= 1 elements, stream-ordered.  From wide_from elements on the three launches run and bsum takes ceil(count / SCAN_BLOCK) + 1 words;
// below it one workgroup walks the array and bsum is not touched.
template <typename Op>
void launch_scan(Op op, int64_t count, int64_t wide_from, uint64_t *bsum, hipStream_t stream) {
  if (count < wide_from) {
    hipLaunchKernelGGL(k_scan_block<Op>, dim3(1), dim3(SCAN_BLOCK), 0, stream, op, (int32_t)count);
    return;
  }
  const int32_t nblk = (int32_t)((count + SCAN_BLOCK - 1) / SCAN_BLOCK);
  hipLaunchKernelGGL(k_scan_sums<Op>, dim3((unsigned)nblk), dim3(SCAN_BLOCK), 0, stream, op, (int32_t)count, bsum);
  hipLaunchKernelGGL(k_scan_block<ScanInPlace>, dim3(1), dim3(SCAN_BLOCK), 0, stream, ScanInPlace{bsum}, nblk);
  hipLaunchKernelGGL(k_scan_apply<Op>, dim3((unsigned)nblk), dim3(SCAN_BLOCK), 0, stream, op, (int32_t)count, bsum);
}

}  // namespace

// a[0 .. P) (P a power of two) sorted by a workgroup of THREADS threads, descending (DESC) or ascending; the array is complete behind a
// barrier of the caller's, and the sort ends with one (P >= 2)
template <bool DESC, int THREADS, typename T>
__device__ __forceinline__ void wg_bitonic_sort(T *a, int P) {
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < (P >> 1); t += THREADS) {
        const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), j = i | stride;
        const T x = a[i], y = a[j];
        if ((DESC ? x < y : x > y) == ((i & size) == 0)) { a[i] = y; a[j] = x; }
      }
      __syncthreads();
    }
}

}  // namespace da
