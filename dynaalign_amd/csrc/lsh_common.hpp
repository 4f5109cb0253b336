// lsh_common.hpp -- what the LSH back end and one-set front end (lsh_kernels.hip) and the two-set front end (lsh_cross_kernels.hip) share:
// the band key, the per-pair decision, and the host-side sizes of the hipcub calls.  Everything here has internal linkage.
#pragma once
#include "da_common.hpp"

#include <algorithm>

#include <hipcub/hipcub.hpp>

namespace da {
namespace {

constexpr int LSH_THREADS = 256;
constexpr int LSH_BAND_SHIFT = 48;            // key = band << 48 | hash >> 16

inline size_t up256(size_t b) { return (b + 255) / 256 * 256; }
inline unsigned lsh_grid(int64_t items) { return (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div(items, LSH_THREADS), 1), 256 * 32); }

// the finaliser of splitmix64: every input bit reaches every output bit
__device__ __forceinline__ uint64_t lsh_mix(uint64_t x) {
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// the bucket key of band t whose `rows` values start at v: the band in the top 16 bits, 48 bits of a hash of the values below
__device__ __forceinline__ unsigned long long lsh_band_key(const uint32_t *__restrict__ v, int rows, int t) {
  uint64_t h = 0x9E3779B97F4A7C15ull;
  for (int c = 0; c < rows; ++c) h = lsh_mix(h + v[c]) + 0x9E3779B97F4A7C15ull;
  return ((unsigned long long)t << LSH_BAND_SHIFT) | (h >> (64 - LSH_BAND_SHIFT));
}

// ---- the per-pair decision --------------------------------------------------------------------------------------------------------------
struct LshVerdict {
  uint32_t count;   // columns h < n_hash with ri[h] == rj[h]
  bool first;       // `band` agrees in all its columns and no earlier band does
};
// Called by a whole wave with wave-uniform arguments; lane l holds column h0 + l of a chunk of 64.  band_cols = bands * rows: the columns
// behind belong to no band but count.  A band agrees when the run of equal columns ending at its last column is at least `rows` long; the
// run is measured inside the chunk from the ballot of mismatches and continued into the chunks before by `tail`, the number of equal
// columns they end with.  Only the first agreeing band is looked for: the candidate (i, j, band) is that pair's own when it is `band`.
__device__ __forceinline__ LshVerdict lsh_pair_decide(const uint32_t *__restrict__ ri, const uint32_t *__restrict__ rj, int n_hash, int band_cols, int rows,
                                                      int band) {
  const int lane = threadIdx.x & 63;
  const unsigned long long upto = (2ull << lane) - 1;   // my column and those below it in the chunk
  const int step = 64 % rows;
  int pos = lane % rows;                                // position of my column in its band
  int tail = 0, first_end = -1;
  uint32_t count = 0;
  for (int h0 = 0; h0 < n_hash; h0 += 64) {
    const int h = h0 + lane;
    const bool eq = h < n_hash && ri[h] == rj[h];
    const unsigned long long equal = __ballot(eq);
    count += (uint32_t)__popcll(equal);
    if (first_end < 0 && h0 < band_cols) {
      const unsigned long long below = ~equal & upto;
      const int run = below ? lane - 63 + __clzll((long long)below) : lane + 1 + tail;
      const unsigned long long agree = __ballot(pos == rows - 1 && h < band_cols && run >= rows);
      if (agree) first_end = h0 + __ffsll((long long)agree) - 1;
    }
    tail = ~equal ? __clzll((long long)~equal) : tail + 64;
    pos += step;
    if (pos >= rows) pos -= rows;
  }
  LshVerdict v;
  v.count = count;
  v.first = first_end == band * rows + rows - 1;
  return v;
}

__device__ __forceinline__ unsigned long long lsh_shfl64(unsigned long long v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
  return ((unsigned long long)hi << 32) | lo;
}

inline int bits_for(int64_t values) {   // bits that hold 0 .. values - 1
  int b = 1;
  while (b < 63 && ((int64_t)1 << b) < values) ++b;
  return b;
}

inline size_t sort_u64_i32_bytes(int64_t items) {
  size_t t = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, t, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, (const int32_t *)nullptr,
                                           (int32_t *)nullptr, (int)items, 0, 64, nullptr);
  return t;
}
inline size_t sort_u64_u16_bytes(int64_t items) {
  size_t t = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, t, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, (const uint16_t *)nullptr,
                                           (uint16_t *)nullptr, (int)items, 0, 64, nullptr);
  return t;
}
inline size_t scan_u32_bytes(int64_t items) {
  size_t t = 0;
  (void)hipcub::DeviceScan::InclusiveSum(nullptr, t, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)items, nullptr);
  return t;
}
inline size_t scan_i64_bytes(int64_t items) {
  size_t t = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t, (const long long *)nullptr, (long long *)nullptr, (int)items, nullptr);
  return t;
}

template <typename T> T *at_bytes(void *base, size_t off) { return reinterpret_cast<T *>(static_cast<char *>(base) + off); }
// the first 256-byte boundary at or behind p: the layouts carry 256 spare bytes for this
template <typename T> T *align256(T *p) { return reinterpret_cast<T *>((reinterpret_cast<uintptr_t>(p) + 255) & ~(uintptr_t)255); }

}  // namespace
}  // namespace da
