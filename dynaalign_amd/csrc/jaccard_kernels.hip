// jaccard_kernels.hip -- the EXACT Jaccard index of two sequences' k-shingle sets (what similarityMH estimates), for short sequences.
//
// S_k(s) is the set of distinct length-k byte substrings of s (byte-wise, as generate_kmers takes them for MinHash; empty when len(s) < k),
// J(a, b) = |S_k(a) n S_k(b)| / |S_k(a) u S_k(b)|, 1.0 when both sets are empty.  The limits of the entry points (k <= 8, at most 127
// shingle positions per sequence) make a shingle one 32- or 64-bit key -- the k bytes big-endian, so key order is byte order -- and a set
// a list of at most 127 keys.
//
// k_jaccard_sets<Key>: one wave per sequence.  The up to 127 keys of its positions go to LDS, two per lane; a key is kept when no earlier
//   position holds the same key, and its place in the output is the number of kept keys below it (two wave-uniform sweeps over the
//   positions, each a broadcast LDS read): the ascending distinct keys at keys[seq * ld_keys + 0 .. count) and count[seq], the slots from
//   count to ld_keys zeroed.  No padding key exists -- FF FF FF FF is a legal shingle -- the counts say where a list ends.
// k_jaccard_rect<Key, KIND>: rows [row_begin, row_end) x columns [col_begin, col_end) of ONE resident set operand in 64 x 64 tiles, tile
//   origins relative to the rectangle's.  A workgroup of four waves stages the key lists of the tile's rows as they lie in memory
//   ([row][slot]) and those of its columns transposed ([slot][column]); each lane owns one column, each wave walks 16 of the rows.  The
//   two-pointer merge of a pair reads the row's key at the lane's row cursor -- lanes at the same cursor share the address, other cursors
//   are other banks of one contiguous list -- and the column's key at [slot][lane], a bank of the lane's own.  It ends after at most
//   ca + cb - 1 steps with the intersection; the union is ca + cb - intersection.
//   DA_OUT_COMPACT: intersection << 8 | union (0x0101 for two empty sets), the tile's codes collected in LDS and stored 8 at a time where
//   the address is 16-byte aligned and all 8 columns exist, singly otherwise.  DA_OUT_F64: (double)intersection / (double)union, 1.0 for
//   two empty sets, one 8-byte store per lane, 512 consecutive bytes per wave and row.
//   A rectangle whose rows and columns are the same range is symmetric: only the tiles on and above the diagonal are launched, and a tile off the
//   diagonal is stored twice, as it is and transposed, from its codes in LDS (the transposed doubles are the code's own divide, 1 / 1 for 0x0101).
//   No atomics, no scratch, every element of the rectangle written exactly once, nothing outside it touched.
#include "da_common.hpp"
#include "jaccard_common.hpp"

namespace da {
namespace {

constexpr int JC_THREADS = 256;
constexpr int JC_TILE = 64;                   // rows and columns of a tile; one lane per column
constexpr int JC_WAVES = JC_THREADS / 64;
constexpr int JC_ROWS_PER_WAVE = JC_TILE / JC_WAVES;
constexpr int JC_MAX_SHINGLES = 127;          // positions per sequence: the union of a pair fits the code's low byte
constexpr int JC_SLOTS = 128;                 // two per lane
constexpr int JC_SO_LD = 72;                  // row stride of the tile's codes in LDS: rows stay 16-byte aligned, a column's rows spread over 8 banks

template <typename Key>
__global__ __launch_bounds__(JC_THREADS) void k_jaccard_sets(const uint8_t *__restrict__ res, const int64_t *__restrict__ off, int64_t n, int k,
                                                             Key *__restrict__ keys, int ld_keys, uint8_t *__restrict__ counts) {
  __shared__ Key sk[JC_WAVES][JC_SLOTS];
  __shared__ uint8_t sfirst[JC_WAVES][JC_SLOTS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t s = (int64_t)blockIdx.x * JC_WAVES + wave;
  const bool live = s < n;                                              // (the last workgroup's spare waves keep the barriers company)
  const int64_t b0 = live ? off[s] : 0;
  const int64_t len = live ? off[s + 1] - b0 : 0;
  int np = len >= k ? (int)(len - k + 1 < JC_MAX_SHINGLES ? len - k + 1 : JC_MAX_SHINGLES) : 0;
  if (np > ld_keys) np = ld_keys;                                       // (the launcher refuses such a call: nothing is written past a row)
  Key mine[2] = {0, 0};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int q = lane + 64 * h;
    if (q < np) {
      Key v = 0;
      for (int b = 0; b < k; ++b) v = (Key)(v << 8) | (Key)res[b0 + q + b];
      mine[h] = v;
      sk[wave][q] = v;
    }
  }
  __syncthreads();
  // a position is kept when no earlier position holds its key
  bool first[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int q = lane + 64 * h;
    bool f = q < np;
    for (int p = 0; p < np; ++p) f = f && !(p < q && sk[wave][p] == mine[h]);
    first[h] = f;
    if (q < np) sfirst[wave][q] = f ? 1 : 0;
  }
  __syncthreads();
  if (!live) return;
  const int count = __popcll(__ballot(first[0])) + __popcll(__ballot(first[1]));
  Key *row = keys + s * (int64_t)ld_keys;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    int rank = 0;
    for (int p = 0; p < np; ++p) rank += (sfirst[wave][p] != 0 && sk[wave][p] < mine[h]) ? 1 : 0;
    if (first[h]) row[rank] = mine[h];                                 // rank < count <= np <= ld_keys
  }
  for (int q = count + lane; q < ld_keys; q += 64) row[q] = 0;
  if (lane == 0) counts[s] = (uint8_t)count;
}

template <typename Key, int KIND>
__global__ __launch_bounds__(JC_THREADS) void k_jaccard_rect(const Key *__restrict__ keys, const uint8_t *__restrict__ counts, int ld_keys,
                                                             int64_t row_begin, int64_t row_end, int64_t col_begin, int64_t col_end,
                                                             void *__restrict__ out, int64_t ld, int tiles_c, int sym) {
  extern __shared__ __attribute__((aligned(16))) unsigned char jc_lds[];
  Key *sc = reinterpret_cast<Key *>(jc_lds);                            // [ld_keys][64]: slot-major, the lane's column at [slot][lane]
  Key *sr = sc + (size_t)ld_keys * JC_TILE;                             // [64][ld_keys]: the rows as they lie in memory
  uint16_t *so = reinterpret_cast<uint16_t *>(sr + (size_t)ld_keys * JC_TILE);   // [64][JC_SO_LD] codes of the tile
  uint8_t *sca = reinterpret_cast<uint8_t *>(so + JC_TILE * JC_SO_LD);
  uint8_t *scb = sca + JC_TILE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int tr, tc;
  if (sym) jc_upper_tile(blockIdx.x, tiles_c, tr, tc);
  else { tr = (int)(blockIdx.x / (unsigned)tiles_c); tc = (int)(blockIdx.x % (unsigned)tiles_c); }
  const bool mirror = sym && tr != tc;                                  // J is symmetric: this tile is also the transpose of tile (tc, tr)
  const int64_t r0 = row_begin + (int64_t)tr * JC_TILE;
  const int64_t c0 = col_begin + (int64_t)tc * JC_TILE;
  const int nr = (int)(row_end - r0 < JC_TILE ? row_end - r0 : JC_TILE);
  const int nc = (int)(col_end - c0 < JC_TILE ? col_end - c0 : JC_TILE);
  if (tid < JC_TILE) sca[tid] = tid < nr ? counts[r0 + tid] : 0;
  else if (tid < 2 * JC_TILE) scb[tid - JC_TILE] = tid - JC_TILE < nc ? counts[c0 + tid - JC_TILE] : 0;
  {
    const Key *src = keys + r0 * (int64_t)ld_keys;
    const int total = nr * ld_keys;
    for (int e = tid; e < total; e += JC_THREADS) sr[e] = src[e];
  }
  for (int e = tid; e < ld_keys * JC_TILE; e += JC_THREADS) {
    const int col = e & (JC_TILE - 1), slot = e >> 6;
    if (col < nc) sc[e] = keys[(c0 + col) * (int64_t)ld_keys + slot];
  }
  __syncthreads();
  const int cb = scb[lane];
  const Key *mycol = sc + lane;
#pragma unroll 1
  for (int rr = 0; rr < JC_ROWS_PER_WAVE; ++rr) {
    const int r = wave * JC_ROWS_PER_WAVE + rr;
    if (r >= nr) break;                                                 // wave-uniform
    const int ca = sca[r];
    const Key *rowk = sr + r * ld_keys;
    int i = 0, j = 0, inter = 0;
    while (i < ca && j < cb) {
      const Key a = rowk[i], b = mycol[j * JC_TILE];
      inter += a == b ? 1 : 0;
      i += a <= b ? 1 : 0;
      j += b <= a ? 1 : 0;
    }
    const int uni = ca + cb - inter;
    if (KIND == DA_OUT_COMPACT || mirror) so[r * JC_SO_LD + lane] = (uint16_t)(uni ? (inter << 8) | uni : 0x0101);
    if (KIND == DA_OUT_F64 && lane < nc)
      static_cast<double *>(out)[(r0 + r - row_begin) * ld + (c0 - col_begin) + lane] = uni ? (double)inter / (double)uni : 1.0;
  }
  if (KIND != DA_OUT_COMPACT && !mirror) return;                        // workgroup-uniform
  __syncthreads();
  if (KIND == DA_OUT_COMPACT) {
    uint16_t *o16 = static_cast<uint16_t *>(out);
#pragma unroll
    for (int h = 0; h < JC_TILE * JC_TILE / 8 / JC_THREADS; ++h) {
      const int q = tid + JC_THREADS * h, r = q >> 3, c = (q & 7) * 8;
      if (r >= nr || c >= nc) continue;
      uint16_t *dst = o16 + (r0 + r - row_begin) * ld + (c0 - col_begin) + c;
      const uint16_t *srcv = so + r * JC_SO_LD + c;
      if (c + 8 <= nc && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<const uint4 *>(srcv);
      } else {
        const int m = nc - c < 8 ? nc - c : 8;
        for (int e = 0; e < m; ++e) dst[e] = srcv[e];
      }
    }
    if (mirror) {                                                       // element (c0 + c, r0 + r) = code of (r0 + r, c0 + c): 8 rows of one column
#pragma unroll
      for (int h = 0; h < JC_TILE * JC_TILE / 8 / JC_THREADS; ++h) {
        const int q = tid + JC_THREADS * h, c = q >> 3, r = (q & 7) * 8;
        if (c >= nc || r >= nr) continue;
        uint16_t *dst = o16 + (c0 + c - row_begin) * ld + (r0 - col_begin) + r;
        const uint16_t *srcv = so + r * JC_SO_LD + c;
        const int m = nr - r < 8 ? nr - r : 8;
        if (m == 8 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
          uint4 v;
          v.x = (uint32_t)srcv[0] | (uint32_t)srcv[JC_SO_LD] << 16;
          v.y = (uint32_t)srcv[2 * JC_SO_LD] | (uint32_t)srcv[3 * JC_SO_LD] << 16;
          v.z = (uint32_t)srcv[4 * JC_SO_LD] | (uint32_t)srcv[5 * JC_SO_LD] << 16;
          v.w = (uint32_t)srcv[6 * JC_SO_LD] | (uint32_t)srcv[7 * JC_SO_LD] << 16;
          *reinterpret_cast<uint4 *>(dst) = v;
        } else {
          for (int e = 0; e < m; ++e) dst[e] = srcv[e * JC_SO_LD];
        }
      }
    }
  } else {                                                              // DA_OUT_F64, mirror: consecutive lanes store consecutive columns
    double *o64 = static_cast<double *>(out);
    if (lane < nr) {
#pragma unroll 4
      for (int cc = 0; cc < JC_ROWS_PER_WAVE; ++cc) {
        const int c = wave * JC_ROWS_PER_WAVE + cc;
        if (c >= nc) break;
        const unsigned code = so[lane * JC_SO_LD + c];                  // 0x0101 for two empty sets: 1 / 1, the 1.0 of the direct store
        o64[(c0 + c - row_begin) * ld + (r0 - col_begin) + lane] = (double)(code >> 8) / (double)(code & 255u);
      }
    }
  }
}

template <typename Key> size_t jc_rect_lds(int ld_keys) {
  return (size_t)2 * ld_keys * JC_TILE * sizeof(Key) + (size_t)JC_TILE * JC_SO_LD * sizeof(uint16_t) + 2 * JC_TILE;
}

template <typename Key, int KIND>
int jc_launch_rect(const void *d_keys, const uint8_t *d_counts, int ld_keys, int64_t r0, int64_t r1, int64_t c0, int64_t c1, void *d_out, int64_t ld,
                   hipStream_t stream) {
  const int64_t tr = ceil_div(r1 - r0, JC_TILE), tc = ceil_div(c1 - c0, JC_TILE);
  // rows and columns are the same range: the tiles on and above the diagonal are computed and each is stored twice, as it is and transposed
  const bool sym = r0 == c0 && r1 == c1 && tr > 1;
  const int64_t tiles = sym ? tr * (tr + 1) / 2 : tr * tc;
  if (tiles > 0x7fffffffLL || tc > 0x3fffffffLL) return fail(DA_ERR_UNSUPPORTED, "exact Jaccard: rectangle too large for one launch");
  const size_t dyn = jc_rect_lds<Key>(ld_keys);
  if (dyn > 48 * 1024) {   // above the default limit of a launch: 127 shingles take up to 137 KiB of the CU's 160 KiB
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_jaccard_rect<Key, KIND>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
    if (e != hipSuccess) return fail(DA_ERR_HIP, "hipFuncSetAttribute(k_jaccard_rect, %zu bytes of LDS) failed: %s", dyn, hipGetErrorString(e));
  }
  hipLaunchKernelGGL((k_jaccard_rect<Key, KIND>), dim3((unsigned)tiles), dim3(JC_THREADS), dyn, stream, static_cast<const Key *>(d_keys), d_counts,
                     ld_keys, r0, r1, c0, c1, d_out, ld, (int)tc, sym ? 1 : 0);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

}  // namespace

int64_t jaccard_sets_ld(int64_t max_len, int k) {
  if (k < 1) return 0;
  const int64_t np = max_len >= k ? max_len - k + 1 : 0;
  return np <= 4 ? 4 : (np + 3) / 4 * 4;
}

int launch_jaccard_sets(const uint8_t *d_res, const int64_t *d_off, int64_t n, int64_t max_len, int k, void *d_keys, int64_t ld_keys, uint8_t *d_counts,
                        hipStream_t stream) {
  if (!d_res || !d_off || !d_keys || !d_counts) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (n < 0 || max_len < 0) return fail(DA_ERR_BAD_ARG, "negative shape");
  if (k < 1 || k > 8) return fail(DA_ERR_BAD_ARG, "k must be in 1 .. 8 (got %d)", k);
  if (max_len - k + 1 > JC_MAX_SHINGLES) return fail(DA_ERR_BAD_ARG, "at most %d shingle positions per sequence (max_len - k + 1 = %lld)", JC_MAX_SHINGLES, (long long)(max_len - k + 1));
  if (ld_keys < jaccard_sets_ld(max_len, k) || ld_keys > JC_SLOTS)
    return fail(DA_ERR_BAD_ARG, "ld_keys (%lld) must be in da_dev_jaccard_sets_ld(max_len, k) = %lld .. %d", (long long)ld_keys, (long long)jaccard_sets_ld(max_len, k), JC_SLOTS);
  if (reinterpret_cast<uintptr_t>(d_keys) & (k <= 4 ? 3 : 7)) return fail(DA_ERR_BAD_ARG, "key buffer must be aligned to its %d-byte keys", k <= 4 ? 4 : 8);
  if (n == 0) return DA_OK;
  if (ceil_div(n, JC_WAVES) > 0x7fffffffLL) return fail(DA_ERR_UNSUPPORTED, "exact Jaccard: too many sequences for one launch");
  const dim3 grid((unsigned)ceil_div(n, JC_WAVES));
  if (k <= 4)
    hipLaunchKernelGGL(k_jaccard_sets<uint32_t>, grid, dim3(JC_THREADS), 0, stream, d_res, d_off, n, k, static_cast<uint32_t *>(d_keys), (int)ld_keys, d_counts);
  else
    hipLaunchKernelGGL(k_jaccard_sets<uint64_t>, grid, dim3(JC_THREADS), 0, stream, d_res, d_off, n, k, static_cast<uint64_t *>(d_keys), (int)ld_keys, d_counts);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

int launch_jaccard_rect(const void *d_keys, const uint8_t *d_counts, int64_t n, int64_t ld_keys, int k, int64_t row_begin, int64_t row_end, int64_t col_begin,
                        int64_t col_end, int kind, void *d_out, int64_t ld, hipStream_t stream) {
  if (!d_keys || !d_counts || !d_out) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (n < 0) return fail(DA_ERR_BAD_ARG, "negative shape");
  if (k < 1 || k > 8) return fail(DA_ERR_BAD_ARG, "k must be in 1 .. 8 (got %d)", k);
  if (ld_keys < 1 || ld_keys > JC_SLOTS) return fail(DA_ERR_BAD_ARG, "ld_keys must be in 1 .. %d (got %lld)", JC_SLOTS, (long long)ld_keys);
  if (row_begin < 0 || row_end > n || row_begin > row_end) return fail(DA_ERR_BAD_ARG, "bad row range");
  if (col_begin < 0 || col_end > n || col_begin > col_end) return fail(DA_ERR_BAD_ARG, "bad column range");
  if (ld < col_end - col_begin) return fail(DA_ERR_BAD_ARG, "ld (%lld) < columns (%lld)", (long long)ld, (long long)(col_end - col_begin));
  if (kind != DA_OUT_F64 && kind != DA_OUT_COMPACT) return fail(DA_ERR_BAD_ARG, "bad output kind");
  if (reinterpret_cast<uintptr_t>(d_keys) & (k <= 4 ? 3 : 7)) return fail(DA_ERR_BAD_ARG, "key buffer must be aligned to its %d-byte keys", k <= 4 ? 4 : 8);
  if (reinterpret_cast<uintptr_t>(d_out) & (kind == DA_OUT_F64 ? 7 : 1)) return fail(DA_ERR_BAD_ARG, "output must be naturally aligned");
  if (row_begin == row_end || col_begin == col_end) return DA_OK;
  if (k <= 4)
    return kind == DA_OUT_COMPACT
               ? jc_launch_rect<uint32_t, DA_OUT_COMPACT>(d_keys, d_counts, (int)ld_keys, row_begin, row_end, col_begin, col_end, d_out, ld, stream)
               : jc_launch_rect<uint32_t, DA_OUT_F64>(d_keys, d_counts, (int)ld_keys, row_begin, row_end, col_begin, col_end, d_out, ld, stream);
  return kind == DA_OUT_COMPACT ? jc_launch_rect<uint64_t, DA_OUT_COMPACT>(d_keys, d_counts, (int)ld_keys, row_begin, row_end, col_begin, col_end, d_out, ld, stream)
                                : jc_launch_rect<uint64_t, DA_OUT_F64>(d_keys, d_counts, (int)ld_keys, row_begin, row_end, col_begin, col_end, d_out, ld, stream);
}

}  // namespace da
