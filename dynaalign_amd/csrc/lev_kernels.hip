// lev_kernels.hip -- the Levenshtein (unit-cost edit) distance of two byte strings in its bit-parallel form (Myers 1999, Hyyro's global
// variant), for sequences of at most 127 bytes.
//
// d(a, b): insert, delete and substitute cost 1 each.  L = max(len(a), len(b)); the similarity is (double)(L - d) / (double)L, 1.0 for two
// empty strings.  A whole column of the DP lives in one or two machine words: a pair costs len(b) steps of some seventeen integer
// operations in place of len(a) * len(b) cells.  The word shape is chosen once per call from max_len -- one uint32 (<= 32), one uint64
// (<= 64), two uint64 (<= 127) -- and is a template parameter of both kernels.
//
// The bytes that occur in a call are mapped to dense class ids 0 .. C-1 (C <= 256, the 256-entry map is a kernel argument), so that a
// sequence's match masks take C entries and not 256.  The operand of a call is ONE buffer of lev_masks_bytes(n, max_len, C) bytes:
//   peq   [n][C][NW] words: bit p % B of word p / B of peq[s][c] is set iff byte p of sequence s has class c
//   text  [n][ld_text] bytes, ld_text = max_len rounded up to a multiple of 4 (at least 4): the class ids, zero past the end
//   len   [n] bytes
// k_lev_masks<Word, NW>: one wave per sequence.  Its class ids go to LDS; a lane builds the words of the classes lane, lane + 64, ...
// k_lev_rect<Word, NW, KIND>: rows [row_begin, row_end) x columns [col_begin, col_end) in 64 x 64 tiles, tile origins relative to the
//   rectangle's.  The row sequence is the pattern, the column sequence the text.  Each lane owns one column: the tile's column texts lie in
//   LDS four steps to a dword, [dword][lane], a bank of the lane's own.  The peq tables of the rows are staged in LDS `rows_staged` at a time
//   (all 64 where they fit the budget); each of the four waves takes staged rows in turn, and a step reads the row's word of the lane's class:
//   lanes of one class share the address, other classes are other banks of one short table.  A lane runs its own text length, shorter
//   lanes idle; the staging loops and barriers are workgroup-uniform.
//   DA_OUT_COMPACT: (L - d) << 8 | L (0x0101 for two empty strings), the tile's codes collected in LDS and stored 8 at a time where the
//   address is 16-byte aligned and all 8 columns exist, singly otherwise.  DA_OUT_F64: one 8-byte store per lane, 512 consecutive bytes per
//   wave and row.  A rectangle whose rows and columns are the same range is symmetric: only the tiles on and above the diagonal are launched,
//   and a tile off the diagonal is stored twice, as it is and transposed, from its codes in LDS.
//   No atomics, no scratch, every element of the rectangle written exactly once, nothing outside it touched.
#include "da_common.hpp"
#include "jaccard_common.hpp"

namespace da {
namespace {

constexpr int LV_THREADS = 256;
constexpr int LV_TILE = 64;                   // rows and columns of a tile; one lane per column
constexpr int LV_WAVES = LV_THREADS / 64;
constexpr int LV_MAX_LEN = 127;               // bytes per sequence: L fits the code's low byte, L - d its high byte
constexpr int LV_SO_LD = 72;                  // row stride of the tile's codes in LDS: rows stay 16-byte aligned, a column's rows spread over 8 banks
constexpr size_t LV_LDS_BUDGET = 64 * 1024;   // of the CU's 160 KiB: two workgroups share a CU whatever the alphabet

struct LevMap { uint8_t v[256]; };            // byte -> class id

// the column of the DP as bit vectors: NW words of B bits, word 0 the low one
template <typename Word, int NW> struct LevColumn;

template <typename Word> struct LevColumn<Word, 1> {
  Word pv, mv;
  __device__ __forceinline__ void init() { pv = ~(Word)0; mv = 0; }
  // one text byte whose match mask is eq; returns +1 / 0 / -1, the change of the score at the pattern's last bit
  __device__ __forceinline__ int step(const Word *eqp, int last) {
    const Word eq = eqp[0];
    const Word xv = eq | mv;
    const Word xh = (((eq & pv) + pv) ^ pv) | eq;
    Word ph = mv | ~(xh | pv);
    Word mh = pv & xh;
    const int delta = (int)((ph >> last) & 1) - (int)((mh >> last) & 1);
    ph = (ph << 1) | 1;
    mh = mh << 1;
    pv = mh | ~(xv | ph);
    mv = ph & xv;
    return delta;
  }
};

template <typename Word> struct LevColumn<Word, 2> {
  static constexpr int B = 8 * (int)sizeof(Word);
  Word pv0, pv1, mv0, mv1;
  __device__ __forceinline__ void init() { pv0 = pv1 = ~(Word)0; mv0 = mv1 = 0; }
  __device__ __forceinline__ int step(const Word *eqp, int last) {
    const Word eq0 = eqp[0], eq1 = eqp[1];
    const Word xv0 = eq0 | mv0, xv1 = eq1 | mv1;
    const Word a0 = eq0 & pv0, a1 = eq1 & pv1;
    const Word s0 = a0 + pv0;
    const Word s1 = a1 + pv1 + (Word)(s0 < a0 ? 1 : 0);               // the addition carries from word 0 into word 1
    const Word xh0 = (s0 ^ pv0) | eq0, xh1 = (s1 ^ pv1) | eq1;
    Word ph0 = mv0 | ~(xh0 | pv0), ph1 = mv1 | ~(xh1 | pv1);
    Word mh0 = pv0 & xh0, mh1 = pv1 & xh1;
    const Word phl = last >= B ? ph1 : ph0, mhl = last >= B ? mh1 : mh0;   // `last` is wave-uniform
    const int delta = (int)((phl >> (last & (B - 1))) & 1) - (int)((mhl >> (last & (B - 1))) & 1);
    ph1 = (ph1 << 1) | (ph0 >> (B - 1));                              // both shifts carry the top bit of word 0 into bit 0 of word 1
    ph0 = (ph0 << 1) | 1;                                             // the shifted-in 1 belongs to word 0 only
    mh1 = (mh1 << 1) | (mh0 >> (B - 1));
    mh0 = mh0 << 1;
    pv0 = mh0 | ~(xv0 | ph0); pv1 = mh1 | ~(xv1 | ph1);
    mv0 = ph0 & xv0; mv1 = ph1 & xv1;
    return delta;
  }
};

// where the three parts of the operand buffer lie
struct LevLayout {
  int ld_text;
  size_t text_at, len_at, bytes;
};
template <typename Word, int NW> LevLayout lev_layout(int64_t n, int64_t max_len, int n_classes) {
  LevLayout l;
  l.ld_text = (int)(max_len <= 4 ? 4 : (max_len + 3) / 4 * 4);
  l.text_at = (size_t)n * (size_t)n_classes * NW * sizeof(Word);
  l.len_at = l.text_at + (size_t)n * (size_t)l.ld_text;
  l.bytes = l.len_at + (size_t)n;
  return l;
}

template <typename Word, int NW>
__global__ __launch_bounds__(LV_THREADS) void k_lev_masks(const uint8_t *__restrict__ res, const int64_t *__restrict__ off, int64_t n, LevMap map,
                                                          int n_classes, Word *__restrict__ peq, uint8_t *__restrict__ text, int ld_text,
                                                          uint8_t *__restrict__ lens) {
  constexpr int B = 8 * (int)sizeof(Word);
  __shared__ uint8_t scls[LV_WAVES][128];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t s = (int64_t)blockIdx.x * LV_WAVES + wave;
  const bool live = s < n;                                              // (the last workgroup's spare waves keep the barrier company)
  const int64_t b0 = live ? off[s] : 0;
  const int64_t bytes = live ? off[s + 1] - b0 : 0;
  int len = (int)(bytes < LV_MAX_LEN ? bytes : LV_MAX_LEN);
  if (len > ld_text) len = ld_text;                                     // (the callers refuse such a sequence: nothing is written past a row)
  if (len > B * NW) len = B * NW;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int q = lane + 64 * h;
    const uint8_t c = q < len ? map.v[res[b0 + q]] : 0;
    scls[wave][q] = c;
    if (live && q < ld_text) text[s * (int64_t)ld_text + q] = c;
  }
  __syncthreads();
  if (!live) return;
  if (lane == 0) lens[s] = (uint8_t)len;
  for (int c = lane; c < n_classes; c += 64) {
    Word w[NW];
#pragma unroll
    for (int t = 0; t < NW; ++t) {
      Word m = 0;
      const int end = len - t * B < B ? len - t * B : B;
      for (int p = 0; p < end; ++p) m |= (Word)(scls[wave][t * B + p] == c ? 1 : 0) << p;
      w[t] = m;
    }
#pragma unroll
    for (int t = 0; t < NW; ++t) peq[(s * (int64_t)n_classes + c) * NW + t] = w[t];
  }
}

template <typename Word, int NW, int KIND>
__global__ __launch_bounds__(LV_THREADS) void k_lev_rect(const Word *__restrict__ peq, const uint32_t *__restrict__ text, const uint8_t *__restrict__ lens,
                                                         int n_classes, int ld_text, int rows_staged, int64_t row_begin, int64_t row_end,
                                                         int64_t col_begin, int64_t col_end, void *__restrict__ out, int64_t ld, int tiles_c, int sym) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lv_lds[];
  uint16_t *so = reinterpret_cast<uint16_t *>(lv_lds);                  // [64][LV_SO_LD] codes of the tile
  uint32_t *st = reinterpret_cast<uint32_t *>(so + LV_TILE * LV_SO_LD); // [ld_text / 4][64]: four steps of the lane's column at [dword][lane]
  uint8_t *sca = reinterpret_cast<uint8_t *>(st + (ld_text / 4) * LV_TILE);
  uint8_t *scb = sca + LV_TILE;
  Word *sp = reinterpret_cast<Word *>(scb + LV_TILE);                   // [rows_staged][n_classes][NW]: the staged rows' match masks
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row_words = n_classes * NW;
  int tr, tc;
  if (sym) jc_upper_tile(blockIdx.x, tiles_c, tr, tc);
  else { tr = (int)(blockIdx.x / (unsigned)tiles_c); tc = (int)(blockIdx.x % (unsigned)tiles_c); }
  const bool mirror = sym && tr != tc;                                  // d is symmetric: this tile is also the transpose of tile (tc, tr)
  const int64_t r0 = row_begin + (int64_t)tr * LV_TILE;
  const int64_t c0 = col_begin + (int64_t)tc * LV_TILE;
  const int nr = (int)(row_end - r0 < LV_TILE ? row_end - r0 : LV_TILE);
  const int nc = (int)(col_end - c0 < LV_TILE ? col_end - c0 : LV_TILE);
  if (tid < LV_TILE) sca[tid] = tid < nr ? lens[r0 + tid] : 0;
  else if (tid < 2 * LV_TILE) scb[tid - LV_TILE] = tid - LV_TILE < nc ? lens[c0 + tid - LV_TILE] : 0;
  const int text_words = ld_text / 4;
  for (int e = tid; e < text_words * LV_TILE; e += LV_THREADS) {
    const int col = e & (LV_TILE - 1), q = e >> 6;
    st[e] = col < nc ? text[(c0 + col) * (int64_t)text_words + q] : 0;
  }
#pragma unroll 1
  for (int base = 0; base < nr; base += rows_staged) {                  // workgroup-uniform
    const int cnt = nr - base < rows_staged ? nr - base : rows_staged;
    if (base) __syncthreads();                                          // every wave is done with the rows staged before
    {
      const Word *src = peq + (r0 + base) * (int64_t)row_words;
      const int total = cnt * row_words;
      for (int e = tid; e < total; e += LV_THREADS) sp[e] = src[e];
    }
    __syncthreads();
    const int cb = scb[lane];
#pragma unroll 1
    for (int rr = wave; rr < cnt; rr += LV_WAVES) {                     // wave-uniform
      const int r = base + rr;
      const int ca = sca[r];
      const Word *table = sp + rr * row_words;
      const int last = ca > 0 ? ca - 1 : 0;
      LevColumn<Word, NW> col;
      col.init();
      int score = ca;
      for (int q = 0; 4 * q < cb; ++q) {                                // the lane's own text length; shorter lanes idle
        uint32_t tw = st[q * LV_TILE + lane];
#pragma unroll
        for (int h = 0; h < 4; ++h) {
          if (4 * q + h < cb) score += col.step(table + (tw & 255u) * NW, last);
          tw >>= 8;
        }
      }
      const int d = ca > 0 ? score : cb;                                // an empty pattern: every text byte is an insert
      const int len = ca > cb ? ca : cb;
      if (KIND == DA_OUT_COMPACT || mirror) so[r * LV_SO_LD + lane] = (uint16_t)(len ? ((len - d) << 8) | len : 0x0101);
      if (KIND == DA_OUT_F64 && lane < nc)
        static_cast<double *>(out)[(r0 + r - row_begin) * ld + (c0 - col_begin) + lane] = len ? (double)(len - d) / (double)len : 1.0;
    }
  }
  if (KIND != DA_OUT_COMPACT && !mirror) return;                        // workgroup-uniform
  __syncthreads();
  if (KIND == DA_OUT_COMPACT) {
    uint16_t *o16 = static_cast<uint16_t *>(out);
#pragma unroll
    for (int h = 0; h < LV_TILE * LV_TILE / 8 / LV_THREADS; ++h) {
      const int q = tid + LV_THREADS * h, r = q >> 3, c = (q & 7) * 8;
      if (r >= nr || c >= nc) continue;
      uint16_t *dst = o16 + (r0 + r - row_begin) * ld + (c0 - col_begin) + c;
      const uint16_t *srcv = so + r * LV_SO_LD + c;
      if (c + 8 <= nc && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<const uint4 *>(srcv);
      } else {
        const int m = nc - c < 8 ? nc - c : 8;
        for (int e = 0; e < m; ++e) dst[e] = srcv[e];
      }
    }
    if (mirror) {                                                       // element (c0 + c, r0 + r) = code of (r0 + r, c0 + c): 8 rows of one column
#pragma unroll
      for (int h = 0; h < LV_TILE * LV_TILE / 8 / LV_THREADS; ++h) {
        const int q = tid + LV_THREADS * h, c = q >> 3, r = (q & 7) * 8;
        if (c >= nc || r >= nr) continue;
        uint16_t *dst = o16 + (c0 + c - row_begin) * ld + (r0 - col_begin) + r;
        const uint16_t *srcv = so + r * LV_SO_LD + c;
        const int m = nr - r < 8 ? nr - r : 8;
        if (m == 8 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
          uint4 v;
          v.x = (uint32_t)srcv[0] | (uint32_t)srcv[LV_SO_LD] << 16;
          v.y = (uint32_t)srcv[2 * LV_SO_LD] | (uint32_t)srcv[3 * LV_SO_LD] << 16;
          v.z = (uint32_t)srcv[4 * LV_SO_LD] | (uint32_t)srcv[5 * LV_SO_LD] << 16;
          v.w = (uint32_t)srcv[6 * LV_SO_LD] | (uint32_t)srcv[7 * LV_SO_LD] << 16;
          *reinterpret_cast<uint4 *>(dst) = v;
        } else {
          for (int e = 0; e < m; ++e) dst[e] = srcv[e * LV_SO_LD];
        }
      }
    }
  } else {                                                              // DA_OUT_F64, mirror: consecutive lanes store consecutive columns
    double *o64 = static_cast<double *>(out);
    if (lane < nr) {
#pragma unroll 4
      for (int cc = 0; cc < LV_TILE / LV_WAVES; ++cc) {
        const int c = wave * (LV_TILE / LV_WAVES) + cc;
        if (c >= nc) break;
        const unsigned code = so[lane * LV_SO_LD + c];                  // 0x0101 for two empty strings: 1 / 1, the 1.0 of the direct store
        o64[(c0 + c - row_begin) * ld + (r0 - col_begin) + lane] = (double)(code >> 8) / (double)(code & 255u);
      }
    }
  }
}

// LDS of a rect launch without the staged rows: the tile's codes, the column texts, the two length lists
size_t lev_rect_fixed_lds(int ld_text) { return (size_t)LV_TILE * LV_SO_LD * sizeof(uint16_t) + (size_t)ld_text * LV_TILE + 2 * LV_TILE; }

template <typename Word, int NW>
int lev_launch_masks(const uint8_t *d_res, const int64_t *d_off, int64_t n, int64_t max_len, const LevMap &map, int n_classes, void *d_masks,
                     hipStream_t stream) {
  const LevLayout l = lev_layout<Word, NW>(n, max_len, n_classes);
  unsigned char *base = static_cast<unsigned char *>(d_masks);
  hipLaunchKernelGGL((k_lev_masks<Word, NW>), dim3((unsigned)ceil_div(n, LV_WAVES)), dim3(LV_THREADS), 0, stream, d_res, d_off, n, map, n_classes,
                     reinterpret_cast<Word *>(base), base + l.text_at, l.ld_text, base + l.len_at);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

template <typename Word, int NW, int KIND>
int lev_launch_rect(const void *d_masks, int64_t n, int64_t max_len, int n_classes, int64_t r0, int64_t r1, int64_t c0, int64_t c1, void *d_out,
                    int64_t ld, hipStream_t stream) {
  const LevLayout l = lev_layout<Word, NW>(n, max_len, n_classes);
  const int64_t tr = ceil_div(r1 - r0, LV_TILE), tc = ceil_div(c1 - c0, LV_TILE);
  // rows and columns are the same range: the tiles on and above the diagonal are computed and each is stored twice, as it is and transposed
  const bool sym = r0 == c0 && r1 == c1 && tr > 1;
  const int64_t tiles = sym ? tr * (tr + 1) / 2 : tr * tc;
  if (tiles > 0x7fffffffLL || tc > 0x3fffffffLL) return fail(DA_ERR_UNSUPPORTED, "Levenshtein: rectangle too large for one launch");
  // the rows staged at a time: all 64 of a tile where their tables fit the budget, else a multiple of the four waves (at least 4: 256
  // classes of two uint64 are 4 KiB a row)
  const size_t fixed = lev_rect_fixed_lds(l.ld_text), row_bytes = (size_t)n_classes * NW * sizeof(Word);
  int staged = (int)std::min<size_t>(LV_TILE, (LV_LDS_BUDGET - fixed) / row_bytes);
  staged = std::max(LV_WAVES, staged / LV_WAVES * LV_WAVES);
  const size_t dyn = fixed + (size_t)staged * row_bytes;
  if (dyn > 48 * 1024) {   // above the default limit of a launch
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_lev_rect<Word, NW, KIND>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
    if (e != hipSuccess) return fail(DA_ERR_HIP, "hipFuncSetAttribute(k_lev_rect, %zu bytes of LDS) failed: %s", dyn, hipGetErrorString(e));
  }
  const unsigned char *base = static_cast<const unsigned char *>(d_masks);
  hipLaunchKernelGGL((k_lev_rect<Word, NW, KIND>), dim3((unsigned)tiles), dim3(LV_THREADS), dyn, stream, reinterpret_cast<const Word *>(base),
                     reinterpret_cast<const uint32_t *>(base + l.text_at), base + l.len_at, n_classes, l.ld_text, staged, r0, r1, c0, c1, d_out, ld,
                     (int)tc, sym ? 1 : 0);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

template <typename Word, int NW>
int lev_launch_rect_kind(const void *d_masks, int64_t n, int64_t max_len, int n_classes, int64_t r0, int64_t r1, int64_t c0, int64_t c1, int kind,
                         void *d_out, int64_t ld, hipStream_t stream) {
  return kind == DA_OUT_COMPACT ? lev_launch_rect<Word, NW, DA_OUT_COMPACT>(d_masks, n, max_len, n_classes, r0, r1, c0, c1, d_out, ld, stream)
                                : lev_launch_rect<Word, NW, DA_OUT_F64>(d_masks, n, max_len, n_classes, r0, r1, c0, c1, d_out, ld, stream);
}

int lev_shape_check(int64_t n, int64_t max_len, int n_classes) {
  if (n < 0 || max_len < 0) return fail(DA_ERR_BAD_ARG, "negative shape");
  if (max_len > LV_MAX_LEN) return fail(DA_ERR_UNSUPPORTED, "max_len = %lld: the Levenshtein similarity takes sequences of at most %d bytes", (long long)max_len, LV_MAX_LEN);
  if (n_classes < 1 || n_classes > 256) return fail(DA_ERR_BAD_ARG, "n_classes must be in 1 .. 256 (got %d)", n_classes);
  return DA_OK;
}

}  // namespace

size_t lev_masks_bytes(int64_t n, int64_t max_len, int n_classes) {
  if (n < 0 || max_len < 0 || max_len > LV_MAX_LEN || n_classes < 1 || n_classes > 256) return 0;
  return max_len <= 32 ? lev_layout<uint32_t, 1>(n, max_len, n_classes).bytes
                       : max_len <= 64 ? lev_layout<uint64_t, 1>(n, max_len, n_classes).bytes : lev_layout<uint64_t, 2>(n, max_len, n_classes).bytes;
}

int launch_lev_masks(const uint8_t *d_res, const int64_t *d_off, int64_t n, int64_t max_len, const uint8_t *class_map, int n_classes, void *d_masks,
                     size_t masks_bytes, hipStream_t stream) {
  if (!d_res || !d_off || !class_map || !d_masks) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  int rc;
  if ((rc = lev_shape_check(n, max_len, n_classes)) != DA_OK) return rc;
  LevMap map;
  for (int v = 0; v < 256; ++v) {
    if (class_map[v] >= n_classes) return fail(DA_ERR_BAD_ARG, "class_map[%d] = %d is no class id below n_classes = %d", v, (int)class_map[v], n_classes);
    map.v[v] = class_map[v];
  }
  if (reinterpret_cast<uintptr_t>(d_masks) & 7) return fail(DA_ERR_BAD_ARG, "the mask buffer must be 8-byte aligned");
  if (masks_bytes < lev_masks_bytes(n, max_len, n_classes))
    return fail(DA_ERR_BAD_ARG, "masks_bytes (%zu) < da_dev_lev_masks_bytes(n, max_len, n_classes) = %zu", masks_bytes, lev_masks_bytes(n, max_len, n_classes));
  if (n == 0) return DA_OK;
  if (ceil_div(n, LV_WAVES) > 0x7fffffffLL) return fail(DA_ERR_UNSUPPORTED, "Levenshtein: too many sequences for one launch");
  if (max_len <= 32) return lev_launch_masks<uint32_t, 1>(d_res, d_off, n, max_len, map, n_classes, d_masks, stream);
  if (max_len <= 64) return lev_launch_masks<uint64_t, 1>(d_res, d_off, n, max_len, map, n_classes, d_masks, stream);
  return lev_launch_masks<uint64_t, 2>(d_res, d_off, n, max_len, map, n_classes, d_masks, stream);
}

int launch_lev_rect(const void *d_masks, int64_t n, int64_t max_len, int n_classes, int64_t row_begin, int64_t row_end, int64_t col_begin, int64_t col_end,
                    int kind, void *d_out, int64_t ld, hipStream_t stream) {
  if (!d_masks || !d_out) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  int rc;
  if ((rc = lev_shape_check(n, max_len, n_classes)) != DA_OK) return rc;
  if (row_begin < 0 || row_end > n || row_begin > row_end) return fail(DA_ERR_BAD_ARG, "bad row range");
  if (col_begin < 0 || col_end > n || col_begin > col_end) return fail(DA_ERR_BAD_ARG, "bad column range");
  if (ld < col_end - col_begin) return fail(DA_ERR_BAD_ARG, "ld (%lld) < columns (%lld)", (long long)ld, (long long)(col_end - col_begin));
  if (kind != DA_OUT_F64 && kind != DA_OUT_COMPACT) return fail(DA_ERR_BAD_ARG, "bad output kind");
  if (reinterpret_cast<uintptr_t>(d_masks) & 7) return fail(DA_ERR_BAD_ARG, "the mask buffer must be 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_out) & (kind == DA_OUT_F64 ? 7 : 1)) return fail(DA_ERR_BAD_ARG, "output must be naturally aligned");
  if (row_begin == row_end || col_begin == col_end) return DA_OK;
  if (max_len <= 32) return lev_launch_rect_kind<uint32_t, 1>(d_masks, n, max_len, n_classes, row_begin, row_end, col_begin, col_end, kind, d_out, ld, stream);
  if (max_len <= 64) return lev_launch_rect_kind<uint64_t, 1>(d_masks, n, max_len, n_classes, row_begin, row_end, col_begin, col_end, kind, d_out, ld, stream);
  return lev_launch_rect_kind<uint64_t, 2>(d_masks, n, max_len, n_classes, row_begin, row_end, col_begin, col_end, kind, d_out, ld, stream);
}

}  // namespace da
