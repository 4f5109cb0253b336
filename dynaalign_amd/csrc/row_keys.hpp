// row_keys.hpp -- device helpers the row-walking kernels share (topk_kernels.hip, rect_edges_kernels.hip, nw_edges_long_kernels.hip,
// stats_kernels.hip): a row of keys is taken in chunks of THREADS x PER keys, PER consecutive keys -- one 16-byte load where the row's
// address allows it, single keys otherwise -- per thread.  Every ld and every key-aligned base works.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "scan.hpp"

namespace da {

// KeyRow<Key>::PER: keys per thread per chunk.  load(row, j0, n, vec, k): k[e] = key of column j0 + e of the row for e < nv (the return
// value: how many of the columns [j0, j0 + PER) are < n), 0 beyond; vec: the row starts on a 16-byte boundary.
template <typename Key> struct KeyRow;

template <> struct KeyRow<uint16_t> {
  static constexpr int PER = 8;
  __device__ static __forceinline__ int load(const uint16_t *__restrict__ row, int64_t j0, int64_t n, bool vec, uint32_t k[PER]) {
    int nv;
    if (vec && j0 + PER <= n) {
      const uint4 v = *reinterpret_cast<const uint4 *>(row + j0);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < PER; ++e) k[e] = (w[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu;
      nv = PER;
    } else {
      nv = j0 >= n ? 0 : (n - j0 < PER ? (int)(n - j0) : PER);
#pragma unroll
      for (int e = 0; e < PER; ++e) k[e] = e < nv ? (uint32_t)row[j0 + e] : 0u;
    }
    return nv;
  }
  // the rank a key is ordered by: rank[key], or the key itself without a table (MinHash counts)
  __device__ static __forceinline__ uint32_t rank_of(uint32_t key, const uint16_t *__restrict__ rank) { return rank ? (uint32_t)rank[key] : key; }
  // ... and with the ranks r[e] of the keys that exist (beyond them r[e] = k[e] = 0)
  __device__ static __forceinline__ int load(const uint16_t *__restrict__ row, int64_t j0, int64_t n, bool vec, const uint16_t *__restrict__ rank,
                                             uint32_t r[PER], uint32_t k[PER]) {
    const int nv = load(row, j0, n, vec, k);
#pragma unroll
    for (int e = 0; e < PER; ++e) r[e] = (rank && e < nv) ? (uint32_t)rank[k[e]] : k[e];
    return nv;
  }
};

template <> struct KeyRow<uint32_t> {
  static constexpr int PER = 4;
  __device__ static __forceinline__ int load(const uint32_t *__restrict__ row, int64_t j0, int64_t n, bool vec, uint32_t k[PER]) {
    int nv;
    if (vec && j0 + PER <= n) {
      const uint4 v = *reinterpret_cast<const uint4 *>(row + j0);
      k[0] = v.x; k[1] = v.y; k[2] = v.z; k[3] = v.w;
      nv = PER;
    } else {
      nv = j0 >= n ? 0 : (n - j0 < PER ? (int)(n - j0) : PER);
#pragma unroll
      for (int e = 0; e < PER; ++e) k[e] = e < nv ? row[j0 + e] : 0u;
    }
    return nv;
  }
  // 32-bit keys are value ranks already: the table argument is ignored
  __device__ static __forceinline__ uint32_t rank_of(uint32_t key, const uint16_t *) { return key; }
  __device__ static __forceinline__ int load(const uint32_t *__restrict__ row, int64_t j0, int64_t n, bool vec, const uint16_t *, uint32_t r[PER],
                                             uint32_t k[PER]) {
    const int nv = load(row, j0, n, vec, k);
#pragma unroll
    for (int e = 0; e < PER; ++e) r[e] = k[e];
    return nv;
  }
};

constexpr int TK_PER = KeyRow<uint16_t>::PER;   // uint16 keys per thread per chunk

}  // namespace da
