// jaccard_long_kernels.hip -- the EXACT Jaccard index of two sequences' k-shingle sets for sequences of up to 1024 shingle positions.
//
// The definition is that of jaccard_kernels.hip (S_k(s): the distinct length-k byte substrings of s, J = |A n B| / |A u B|, 1.0 for two empty
// sets, k <= 8: a shingle is one 32- or 64-bit key, the k bytes big-endian, so key order is byte order).  A set is a list of up to 1024
// keys, its count a uint16, and the code of a pair is DA_OUT_PACK32, intersection << 16 | union (1 << 16 | 1 for two empty sets): the shape of
// the long NW code matches << 16 | length, so the value ranks of da_nw_value_ranks(S), S the call's largest shingle count, order it.
//
// k_jaccard_sets_long<Key>: one workgroup of 256 threads per sequence.  The keys of its np <= 1024 positions go to LDS, padded with all-ones
//   keys to the next power of two P; a workgroup bitonic sort of the P keys (wg_bitonic_sort, scan.hpp); the pad keys are not told apart by their value -- FF FF FF FF
//   is a legal shingle -- but by their place: whatever ties with them, the first np sorted keys are the sequence's own.  A key of [0, np) is
//   kept when it differs from its left neighbour, and a workgroup scan of the kept flags (four positions per thread; wg_excl_scan: a wave scan,
//   the four wave totals) gives its slot: the ascending distinct keys at keys[seq * ld_keys + 0 .. count), the row's tail zeroed, counts[seq].
// k_jaccard_rect_long<Key, KIND>: rows [row_begin, row_end) x columns [col_begin, col_end) of ONE resident set operand in 64 x 64 tiles, four
//   waves.  The tile's rows are taken in batches of JL_R = 8: the workgroup stages the batch's lists in LDS ([row][slot], only the count of
//   every list), then each wave takes every fourth column of the tile, reads that column's list from global memory in coalesced chunks of 64
//   keys, one per lane (the next chunk is loaded while this one is searched), and every lane binary-searches its key in each staged row over
//   [0, ca) -- a branch-free lower bound; the eight searches of a batch run in lockstep for the trip count of the batch's longest list, so
//   the loop is wave-uniform and eight independent LDS reads are in flight per step.  The hits of a chunk are a ballot's population
//   count, so the eight intersections of a column are wave-uniform sums and need no reduction; union = ca + cb - intersection.  The work
//   of a pair is cb * log2(ca) LDS reads spread over 64 lanes, and no chain is longer than one search.  The tile's codes are collected in LDS (64 rows of JL_SO_LD words) and stored from
//   there: PACK32 16 bytes at a time where the address is aligned and four columns exist, singly otherwise; F64 as the code's own divide,
//   (double)intersection / (double)union, 512 consecutive bytes per wave and row.
//   A rectangle whose rows and columns are the same range is symmetric: only the tiles on and above the diagonal are launched
//   (jc_upper_tile) and a tile off the diagonal is stored twice, as it is and transposed, from the codes in LDS.
//   No atomics, no scratch, every element of the rectangle written exactly once, nothing outside it touched.
#include "da_common.hpp"
#include "jaccard_common.hpp"
#include "scan.hpp"

namespace da {
namespace {

constexpr int JL_THREADS = 256;
constexpr int JL_TILE = 64;                    // rows and columns of a tile
constexpr int JL_WAVES = JL_THREADS / 64;
constexpr int JL_MAX_SHINGLES = 1024;          // positions per sequence: four per thread of the sets kernel
constexpr int JL_PER = JL_MAX_SHINGLES / JL_THREADS;
constexpr int JL_R = 8;                        // staged rows per batch: 64 KiB of uint64 keys at 1024 shingles
constexpr int JL_SO_LD = 68;                   // row stride of the tile's codes in LDS: rows stay 16-byte aligned, a column's rows spread over 8 banks
constexpr uint32_t JL_EMPTY_PAIR = 1u << 16 | 1u;

template <typename Key>
__global__ __launch_bounds__(JL_THREADS) void k_jaccard_sets_long(const uint8_t *__restrict__ res, const int64_t *__restrict__ off, int64_t n, int k,
                                                                  Key *__restrict__ keys, int ld_keys, uint16_t *__restrict__ counts) {
  __shared__ Key sk[JL_MAX_SHINGLES];
  __shared__ int swave[JL_WAVES];
  const int tid = threadIdx.x;
  const int64_t s = blockIdx.x;                                          // the grid is n workgroups
  const int64_t b0 = off[s];
  const int64_t len = off[s + 1] - b0;
  int np = len >= k ? (int)(len - k + 1 < JL_MAX_SHINGLES ? len - k + 1 : JL_MAX_SHINGLES) : 0;
  if (np > ld_keys) np = ld_keys;                                        // (the launcher refuses such a call: nothing is written past a row)
  int P = 1;
  while (P < np) P <<= 1;
  for (int q = tid; q < P; q += JL_THREADS) {
    Key v = ~(Key)0;                                                     // the pad: never below a real key, so the real ones sort to [0, np)
    if (q < np) {
      v = 0;
      for (int b = 0; b < k; ++b) v = (Key)(v << 8) | (Key)res[b0 + q + b];
    }
    sk[q] = v;
  }
  __syncthreads();
  wg_bitonic_sort<false, JL_THREADS>(sk, P);
  // positions 4 * tid .. 4 * tid + 3: kept when inside [0, np) and different from the left neighbour
  Key mine[JL_PER];
  bool keep[JL_PER];
  int cnt = 0;
#pragma unroll
  for (int e = 0; e < JL_PER; ++e) {
    const int p = tid * JL_PER + e;
    mine[e] = p < np ? sk[p] : (Key)0;
    keep[e] = p < np && (p == 0 || sk[p - 1] != mine[e]);
    cnt += keep[e] ? 1 : 0;
  }
  int total;
  int slot = wg_excl_scan<JL_WAVES>(cnt, swave, &total);
  Key *row = keys + s * (int64_t)ld_keys;
#pragma unroll
  for (int e = 0; e < JL_PER; ++e)
    if (keep[e]) row[slot++] = mine[e];                                  // slot < total <= np <= ld_keys
  for (int q = total + tid; q < ld_keys; q += JL_THREADS) row[q] = 0;
  if (tid == 0) counts[s] = (uint16_t)total;
}

__device__ __forceinline__ double jl_value(uint32_t code) { return (double)(code >> 16) / (double)(code & 0xFFFFu); }   // 1 / 1 for two empty sets

template <typename Key, int KIND>
__global__ __launch_bounds__(JL_THREADS) void k_jaccard_rect_long(const Key *__restrict__ keys, const uint16_t *__restrict__ counts, int ld_keys,
                                                                  int64_t row_begin, int64_t row_end, int64_t col_begin, int64_t col_end,
                                                                  void *__restrict__ out, int64_t ld, int tiles_c, int sym) {
  extern __shared__ __attribute__((aligned(16))) unsigned char jl_lds[];
  uint32_t *so = reinterpret_cast<uint32_t *>(jl_lds);                  // [64][JL_SO_LD] codes of the tile
  int *sca = reinterpret_cast<int *>(so + JL_TILE * JL_SO_LD);          // [64] counts of the tile's rows, 0 past the rectangle
  int *scb = sca + JL_TILE;                                             // [64] ... of its columns
  Key *sr = reinterpret_cast<Key *>(scb + JL_TILE);                     // [JL_R][ld_keys]: the lists of a batch of rows
  const unsigned char *srb = reinterpret_cast<const unsigned char *>(sr);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int tr, tc;
  if (sym) jc_upper_tile(blockIdx.x, tiles_c, tr, tc);
  else { tr = (int)(blockIdx.x / (unsigned)tiles_c); tc = (int)(blockIdx.x % (unsigned)tiles_c); }
  const bool mirror = sym && tr != tc;                                  // J is symmetric: this tile is also the transpose of tile (tc, tr)
  const int64_t r0 = row_begin + (int64_t)tr * JL_TILE;
  const int64_t c0 = col_begin + (int64_t)tc * JL_TILE;
  const int nr = (int)(row_end - r0 < JL_TILE ? row_end - r0 : JL_TILE);
  const int nc = (int)(col_end - c0 < JL_TILE ? col_end - c0 : JL_TILE);
  if (tid < JL_TILE) {                                                  // (a count beyond its row is cut: nothing is read past a list)
    const int c = tid < nr ? (int)counts[r0 + tid] : 0;
    sca[tid] = c < ld_keys ? c : ld_keys;
  } else if (tid < 2 * JL_TILE) {
    const int t = tid - JL_TILE;
    const int c = t < nc ? (int)counts[c0 + t] : 0;
    scb[t] = c < ld_keys ? c : ld_keys;
  }
  __syncthreads();
#pragma unroll 1
  for (int rb = 0; rb < nr; rb += JL_R) {
    if (rb) __syncthreads();                                            // the searches of the previous batch are over
#pragma unroll 1
    for (int q = 0; q < JL_R; ++q) {
      const int ca = sca[rb + q];                                       // rb + q <= 63; 0 for the rows past the rectangle
      const Key *src = keys + (r0 + rb + q) * (int64_t)ld_keys;
      Key *dst = sr + q * ld_keys;
      for (int e = tid; e < ca; e += JL_THREADS) dst[e] = src[e];
    }
    __syncthreads();
    int ca[JL_R], ca_max = 0;                                           // wave-uniform
#pragma unroll
    for (int q = 0; q < JL_R; ++q) {
      ca[q] = sca[rb + q];
      ca_max = ca[q] > ca_max ? ca[q] : ca_max;
    }
#pragma unroll 1
    for (int c = wave; c < nc; c += JL_WAVES) {                         // wave-uniform
      const int cb = scb[c];
      const Key *col = keys + (c0 + c) * (int64_t)ld_keys;
      int hits[JL_R];
#pragma unroll
      for (int q = 0; q < JL_R; ++q) hits[q] = 0;
      Key next = lane < cb ? col[lane] : (Key)0;                        // the chunk after the one being searched is already on its way
#pragma unroll 1
      for (int ch = 0; ch < cb; ch += 64) {
        const bool valid = ch + lane < cb;
        const Key key = next;
        next = ch + 64 + lane < cb ? col[ch + 64 + lane] : (Key)0;
        // the eight searches in lockstep, so that eight LDS reads are in flight: the last key <= `key` of list q lies in [base, base + len);
        // a list that is down to one candidate (half = 0) re-reads it and stays, an empty list reads its unused slot 0 and never counts
        // (base is the byte offset of the candidate in the staged batch: one add, one read, one compare and one select per list and step)
        uint32_t base[JL_R];
        int len[JL_R];
#pragma unroll
        for (int q = 0; q < JL_R; ++q) { base[q] = (uint32_t)(q * ld_keys) * (uint32_t)sizeof(Key); len[q] = ca[q]; }
#pragma unroll 1
        for (int left = ca_max; left > 1; left -= left >> 1) {          // the trip count of the longest list: wave-uniform
#pragma unroll
          for (int q = 0; q < JL_R; ++q) {
            const int half = len[q] >> 1;
            const uint32_t probe = base[q] + (uint32_t)half * (uint32_t)sizeof(Key);
            base[q] = *reinterpret_cast<const Key *>(srb + probe) <= key ? probe : base[q];
            len[q] -= half;
          }
        }
#pragma unroll
        for (int q = 0; q < JL_R; ++q) {
          const bool found = valid && ca[q] > 0 && *reinterpret_cast<const Key *>(srb + base[q]) == key;
          hits[q] += __popcll(__ballot(found));
        }
      }
      int inter = 0;
#pragma unroll
      for (int q = 0; q < JL_R; ++q) inter = lane == q ? hits[q] : inter;
      if (lane < JL_R && rb + lane < nr) {
        const int uni = sca[rb + lane] + cb - inter;
        so[(rb + lane) * JL_SO_LD + c] = uni ? ((uint32_t)inter << 16 | (uint32_t)uni) : JL_EMPTY_PAIR;
      }
    }
  }
  __syncthreads();
  if (KIND == DA_OUT_PACK32) {
    uint32_t *o32 = static_cast<uint32_t *>(out);
#pragma unroll
    for (int h = 0; h < JL_TILE * JL_TILE / 4 / JL_THREADS; ++h) {
      const int q = tid + JL_THREADS * h, r = q >> 4, c = (q & 15) * 4;
      if (r >= nr || c >= nc) continue;
      uint32_t *dst = o32 + (r0 + r - row_begin) * ld + (c0 - col_begin) + c;
      const uint32_t *srcv = so + r * JL_SO_LD + c;
      if (c + 4 <= nc && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<const uint4 *>(srcv);
      } else {
        const int m = nc - c < 4 ? nc - c : 4;
        for (int e = 0; e < m; ++e) dst[e] = srcv[e];
      }
    }
    if (mirror) {                                                       // element (c0 + c, r0 + r) = code of (r0 + r, c0 + c): 4 rows of one column
#pragma unroll
      for (int h = 0; h < JL_TILE * JL_TILE / 4 / JL_THREADS; ++h) {
        const int q = tid + JL_THREADS * h, c = q >> 4, r = (q & 15) * 4;
        if (c >= nc || r >= nr) continue;
        uint32_t *dst = o32 + (c0 + c - row_begin) * ld + (r0 - col_begin) + r;
        const uint32_t *srcv = so + r * JL_SO_LD + c;
        const int m = nr - r < 4 ? nr - r : 4;
        if (m == 4 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
          uint4 v;
          v.x = srcv[0]; v.y = srcv[JL_SO_LD]; v.z = srcv[2 * JL_SO_LD]; v.w = srcv[3 * JL_SO_LD];
          *reinterpret_cast<uint4 *>(dst) = v;
        } else {
          for (int e = 0; e < m; ++e) dst[e] = srcv[e * JL_SO_LD];
        }
      }
    }
  } else {                                                              // DA_OUT_F64: consecutive lanes store consecutive columns
    double *o64 = static_cast<double *>(out);
#pragma unroll 4
    for (int e = tid; e < JL_TILE * JL_TILE; e += JL_THREADS) {
      const int r = e >> 6, c = e & 63;
      if (r < nr && c < nc) o64[(r0 + r - row_begin) * ld + (c0 - col_begin) + c] = jl_value(so[r * JL_SO_LD + c]);
    }
    if (mirror) {
#pragma unroll 4
      for (int e = tid; e < JL_TILE * JL_TILE; e += JL_THREADS) {
        const int c = e >> 6, r = e & 63;
        if (r < nr && c < nc) o64[(c0 + c - row_begin) * ld + (r0 - col_begin) + r] = jl_value(so[r * JL_SO_LD + c]);
      }
    }
  }
}

template <typename Key> size_t jl_rect_lds(int ld_keys) {
  return (size_t)JL_TILE * JL_SO_LD * sizeof(uint32_t) + 2 * JL_TILE * sizeof(int) + (size_t)JL_R * ld_keys * sizeof(Key);
}

template <typename Key, int KIND>
int jl_launch_rect(const void *d_keys, const uint16_t *d_counts, int ld_keys, int64_t r0, int64_t r1, int64_t c0, int64_t c1, void *d_out, int64_t ld,
                   hipStream_t stream) {
  const int64_t tr = ceil_div(r1 - r0, JL_TILE), tc = ceil_div(c1 - c0, JL_TILE);
  // rows and columns are the same range: the tiles on and above the diagonal are computed and each is stored twice, as it is and transposed
  const bool sym = r0 == c0 && r1 == c1 && tr > 1;
  const int64_t tiles = sym ? tr * (tr + 1) / 2 : tr * tc;
  if (tiles > 0x7fffffffLL || tc > 0x3fffffffLL) return fail(DA_ERR_UNSUPPORTED, "exact Jaccard: rectangle too large for one launch");
  const size_t dyn = jl_rect_lds<Key>(ld_keys);
  if (dyn > 48 * 1024) {   // above the default limit of a launch: 1024 uint64 keys a row take 81.5 KiB of the CU's 160 KiB
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_jaccard_rect_long<Key, KIND>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
    if (e != hipSuccess) return fail(DA_ERR_HIP, "hipFuncSetAttribute(k_jaccard_rect_long, %zu bytes of LDS) failed: %s", dyn, hipGetErrorString(e));
  }
  hipLaunchKernelGGL((k_jaccard_rect_long<Key, KIND>), dim3((unsigned)tiles), dim3(JL_THREADS), dyn, stream, static_cast<const Key *>(d_keys), d_counts,
                     ld_keys, r0, r1, c0, c1, d_out, ld, (int)tc, sym ? 1 : 0);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

}  // namespace

int64_t jaccard_sets_long_ld(int64_t max_len, int k) { return jaccard_sets_ld(max_len, k); }   // the largest shingle count rounded up to 4, at least 4

int launch_jaccard_sets_long(const uint8_t *d_res, const int64_t *d_off, int64_t n, int64_t max_len, int k, void *d_keys, int64_t ld_keys,
                             uint16_t *d_counts, hipStream_t stream) {
  if (!d_res || !d_off || !d_keys || !d_counts) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (n < 0 || max_len < 0) return fail(DA_ERR_BAD_ARG, "negative shape");
  if (k < 1 || k > 8) return fail(DA_ERR_BAD_ARG, "k must be in 1 .. 8 (got %d)", k);
  if (max_len - k + 1 > JL_MAX_SHINGLES) return fail(DA_ERR_BAD_ARG, "at most %d shingle positions per sequence (max_len - k + 1 = %lld)", JL_MAX_SHINGLES, (long long)(max_len - k + 1));
  if (ld_keys < jaccard_sets_long_ld(max_len, k) || ld_keys > JL_MAX_SHINGLES)
    return fail(DA_ERR_BAD_ARG, "ld_keys (%lld) must be in da_jaccard_sets_long_ld(max_len, k) = %lld .. %d", (long long)ld_keys, (long long)jaccard_sets_long_ld(max_len, k), JL_MAX_SHINGLES);
  if (reinterpret_cast<uintptr_t>(d_keys) & (k <= 4 ? 3 : 7)) return fail(DA_ERR_BAD_ARG, "key buffer must be aligned to its %d-byte keys", k <= 4 ? 4 : 8);
  if (reinterpret_cast<uintptr_t>(d_counts) & 1) return fail(DA_ERR_BAD_ARG, "count buffer must be aligned to its 2-byte counts");
  if (n == 0) return DA_OK;
  if (n > 0x7fffffffLL) return fail(DA_ERR_UNSUPPORTED, "exact Jaccard: too many sequences for one launch");
  const dim3 grid((unsigned)n);
  if (k <= 4)
    hipLaunchKernelGGL(k_jaccard_sets_long<uint32_t>, grid, dim3(JL_THREADS), 0, stream, d_res, d_off, n, k, static_cast<uint32_t *>(d_keys), (int)ld_keys, d_counts);
  else
    hipLaunchKernelGGL(k_jaccard_sets_long<uint64_t>, grid, dim3(JL_THREADS), 0, stream, d_res, d_off, n, k, static_cast<uint64_t *>(d_keys), (int)ld_keys, d_counts);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

int launch_jaccard_rect_long(const void *d_keys, const uint16_t *d_counts, int64_t n, int64_t ld_keys, int k, int64_t row_begin, int64_t row_end,
                             int64_t col_begin, int64_t col_end, int kind, void *d_out, int64_t ld, hipStream_t stream) {
  if (!d_keys || !d_counts || !d_out) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (n < 0) return fail(DA_ERR_BAD_ARG, "negative shape");
  if (k < 1 || k > 8) return fail(DA_ERR_BAD_ARG, "k must be in 1 .. 8 (got %d)", k);
  if (ld_keys < 1 || ld_keys > JL_MAX_SHINGLES) return fail(DA_ERR_BAD_ARG, "ld_keys must be in 1 .. %d (got %lld)", JL_MAX_SHINGLES, (long long)ld_keys);
  if (row_begin < 0 || row_end > n || row_begin > row_end) return fail(DA_ERR_BAD_ARG, "bad row range");
  if (col_begin < 0 || col_end > n || col_begin > col_end) return fail(DA_ERR_BAD_ARG, "bad column range");
  if (ld < col_end - col_begin) return fail(DA_ERR_BAD_ARG, "ld (%lld) < columns (%lld)", (long long)ld, (long long)(col_end - col_begin));
  if (kind != DA_OUT_F64 && kind != DA_OUT_PACK32) return fail(DA_ERR_BAD_ARG, "bad output kind");
  if (reinterpret_cast<uintptr_t>(d_keys) & (k <= 4 ? 3 : 7)) return fail(DA_ERR_BAD_ARG, "key buffer must be aligned to its %d-byte keys", k <= 4 ? 4 : 8);
  if (reinterpret_cast<uintptr_t>(d_counts) & 1) return fail(DA_ERR_BAD_ARG, "count buffer must be aligned to its 2-byte counts");
  if (reinterpret_cast<uintptr_t>(d_out) & (kind == DA_OUT_F64 ? 7 : 3)) return fail(DA_ERR_BAD_ARG, "output must be naturally aligned");
  if (row_begin == row_end || col_begin == col_end) return DA_OK;
  if (k <= 4)
    return kind == DA_OUT_PACK32
               ? jl_launch_rect<uint32_t, DA_OUT_PACK32>(d_keys, d_counts, (int)ld_keys, row_begin, row_end, col_begin, col_end, d_out, ld, stream)
               : jl_launch_rect<uint32_t, DA_OUT_F64>(d_keys, d_counts, (int)ld_keys, row_begin, row_end, col_begin, col_end, d_out, ld, stream);
  return kind == DA_OUT_PACK32 ? jl_launch_rect<uint64_t, DA_OUT_PACK32>(d_keys, d_counts, (int)ld_keys, row_begin, row_end, col_begin, col_end, d_out, ld, stream)
                               : jl_launch_rect<uint64_t, DA_OUT_F64>(d_keys, d_counts, (int)ld_keys, row_begin, row_end, col_begin, col_end, d_out, ld, stream);
}

}  // namespace da
