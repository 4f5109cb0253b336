// nw_align_kernels.hip -- the alignment PATH of listed pairs (da_nw_align_pairs, da_dev_nw_align_pairs).
//
// The similarity kernels (nw_kernels.hip) carry (matches, length) forward and never know the path.  k_nw_align_fill records, for
// every cell, the decision the reference takes at fill time (src/pairwiseSeqAlign.cpp:271-279) and k_nw_align_walk follows it back
// from (m, n) exactly as the reference's traceback does (:284-308):
//   D  if d >= Ix && d >= Iy (d: the diagonal candidate), else U if Ix >= Iy, else L;   border (i, 0) is U, (0, j) is L.
//
//   * one LANE per listed pair; both sequences are lane-private (0 .. 127 residues each).  Lanes of a wave have their own
//     (m, n): the row and strip loops have lane-private trip counts, so the wave runs to its maximum with finished lanes masked.
//   * the int32 three-state cell of nw_row() (best - goe, Ix; Iy rides along the row): every penalty pair da_similarity_nw takes.
//   * sequence2 is processed in COLUMN STRIPS of 32: a strip's 32 columns of (best - goe, Ix) and the table offsets of its
//     residues are the lane's registers.  The strip's right-hand boundary column -- best - goe and Iy per row; the diagonal
//     neighbour of row r is the boundary of row r - 1 -- waits in the workspace for the next strip.
//   * 2 decision bits per cell (0 D, 1 U, 2 L), 16 cells per word: a row of a strip is two words.  The workspace is laid out
//     [wave][row][word][lane], so the store of one word by the 64 lanes of a wave is 256 consecutive bytes.
//   * the back walk is a second kernel on the same stream with the same pair-to-lane map, so a lane reads the words it wrote (few
//     registers: the walk runs at full occupancy, the fill at what its 96 state registers allow): one pass for length and matches, a
//     second one that fills the ops bytes from the back.  Border steps need no word.  M[m][n] waits in the lane's spare boundary slot.
#include <climits>

#include "da_common.hpp"

namespace da {

const signed char *matrix_table_host(int id);   // nw_kernels.hip

namespace {

struct AlignTable { signed char s[576]; };   // passed by value in the kernarg segment

constexpr int AL_THREADS = 256;
constexpr int AL_STRIP = 32;                                  // columns per strip: two decision words per row
constexpr int AL_MAXLEN = 127;
constexpr int AL_ROWS = 128;                                  // row slots per pair (rows 1 .. 127 use slots 0 .. 126)
constexpr int AL_WORDS = (AL_MAXLEN + 15) / 16;               // decision words per row: 8
constexpr size_t AL_DEC_WORDS = (size_t)AL_ROWS * AL_WORDS * 64;   // per wave
constexpr size_t AL_BND_WORDS = (size_t)AL_ROWS * 2 * 64;          // per wave: (best - goe, Iy) per row
constexpr size_t AL_WAVE_BYTES = (AL_DEC_WORDS + AL_BND_WORDS) * sizeof(uint32_t);   // 5 KiB per pair

// One DP row of a strip for a lane, columns left to right (the cell of nw_row() in nw_kernels.hip without the payload):
//   MG[c] : best[r-1][c] - goe on entry, best[r][c] - goe on exit (best = M after the reference's overwrite, :272-278)
//   X[c]  : Ix[r-1][c] -> Ix[r][c]
// FIRST: row 1, where M[0][c] = Ix[0][c] = NEG (:230-235) while the diagonal still sees Iy[0][c-1] (kept in MG).
// w0 / w1: the row's decisions, cell c at bits 2 (c & 15) of word c >> 4.
template <bool FIRST>
__device__ __forceinline__ void al_row(int32_t (&MG)[AL_STRIP], int32_t (&X)[AL_STRIP], const uint32_t (&boff)[AL_STRIP], const char *tab_row,
                                       int32_t mgd, int32_t mgl, int32_t yl, int32_t ge, int32_t goe, int32_t ix_first, uint32_t &w0,
                                       uint32_t &w1, int32_t &y_last) {
  uint32_t w[2] = {0u, 0u};
#pragma unroll
  for (int c = 0; c < AL_STRIP; ++c) {
    const int32_t e = *reinterpret_cast<const int32_t *>(tab_row + boff[c]);   // score + goe
    const int32_t ix = FIRST ? ix_first : max(MG[c], X[c] - ge);               // reference :255-257
    const int32_t iy = max(mgl, yl - ge);                                      // :260-262
    const int32_t d = mgd + e;                                                 // :265-268
    const int32_t gap = max(ix, iy);
    const bool take_d = d >= gap;                                              // :271
    const bool up_over_left = ix >= iy;                                        // :273
    const uint32_t code = take_d ? 0u : (up_over_left ? 1u : 2u);
    w[c >> 4] |= code << (2 * (c & 15));
    mgd = MG[c];
    mgl = max(d, gap) - goe;                                                   // :272-278 (M overwrite)
    yl = iy;
    MG[c] = mgl;
    X[c] = ix;
  }
  w0 = w[0];
  w1 = w[1];
  y_last = yl;
}

// pair q of this launch: x[pair_x[q]] (sequence1) against y[pair_y[q]] (sequence2); pair_x == NULL: both indices are pair_base + q.
// A pair the kernels cannot take (an index outside its set, a sequence over 127 residues, an ops row too short) gets length -1, matches -1,
// score 0 and no ops: the host call has refused those before, the device-pointer call reports them this way.
struct AlignPair { bool ok; int m, n; const uint8_t *s1, *s2; };
__device__ __forceinline__ AlignPair al_pair(const uint8_t *__restrict__ x_codes, const int64_t *__restrict__ x_off, int64_t m_seqs,
                                             const uint8_t *__restrict__ y_codes, const int64_t *__restrict__ y_off, int64_t n_seqs,
                                             const int32_t *__restrict__ pair_x, const int32_t *__restrict__ pair_y, int64_t pair_base, int64_t q,
                                             bool want_ops, int64_t ld_ops) {
  AlignPair p = {false, 0, 0, nullptr, nullptr};
  const int64_t ix = pair_x ? (int64_t)pair_x[q] : pair_base + q;
  const int64_t iy = pair_y ? (int64_t)pair_y[q] : pair_base + q;
  if (ix < 0 || ix >= m_seqs || iy < 0 || iy >= n_seqs) return p;
  const int64_t b1 = x_off[ix], l1 = x_off[ix + 1] - b1, b2 = y_off[iy], l2 = y_off[iy + 1] - b2;
  if (l1 < 0 || l1 > AL_MAXLEN || l2 < 0 || l2 > AL_MAXLEN || (want_ops && l1 + l2 > ld_ops)) return p;
  p.ok = true; p.m = (int)l1; p.n = (int)l2; p.s1 = x_codes + b1; p.s2 = y_codes + b2;
  return p;
}
__device__ __forceinline__ uint32_t *al_dec(uint32_t *work, int64_t q) {      // [row][word][lane] of the lane's wavefront
  return work + (size_t)(q >> 6) * (AL_DEC_WORDS + AL_BND_WORDS) + (q & 63);
}
__device__ __forceinline__ int32_t *al_bnd(uint32_t *work, int64_t q) {       // [row][2][lane]
  return reinterpret_cast<int32_t *>(work + (size_t)(q >> 6) * (AL_DEC_WORDS + AL_BND_WORDS) + AL_DEC_WORDS) + (q & 63);
}
constexpr size_t AL_SCORE_SLOT = (size_t)(AL_ROWS - 1) * 2 * 64;              // boundary slot of the row no sequence has: M[m][n] for the walk

__global__ __launch_bounds__(AL_THREADS) void k_nw_align_fill(const uint8_t *__restrict__ x_codes, const int64_t *__restrict__ x_off, int64_t m_seqs,
                                                              const uint8_t *__restrict__ y_codes, const int64_t *__restrict__ y_off, int64_t n_seqs,
                                                              const int32_t *__restrict__ pair_x, const int32_t *__restrict__ pair_y,
                                                              int64_t pair_base, int64_t pairs, AlignTable table, int32_t go, int32_t ge, bool want_ops,
                                                              int64_t ld_ops, uint32_t *work) {
  __shared__ __attribute__((aligned(16))) int32_t tab[24 * 24];
  const int32_t goe = go + ge;
  for (int e = threadIdx.x; e < 576; e += AL_THREADS) tab[e] = (int32_t)table.s[e] + goe;
  __syncthreads();

  const int64_t q = (int64_t)blockIdx.x * AL_THREADS + threadIdx.x;
  if (q >= pairs) return;                                  // no barrier below: a lane may leave
  const AlignPair pr = al_pair(x_codes, x_off, m_seqs, y_codes, y_off, n_seqs, pair_x, pair_y, pair_base, q, want_ops, ld_ops);
  if (!pr.ok) return;
  uint32_t *dec = al_dec(work, q);
  int32_t *bnd = al_bnd(work, q);
  const int m = pr.m, n = pr.n;
  const uint8_t *s1 = pr.s1, *s2 = pr.s2;
  const int32_t NEG = INT_MIN / 2;
  const int32_t ix_first = max(NEG - goe, NEG - ge);
  const char *tab_bytes = reinterpret_cast<const char *>(tab);

  // strips of 32 columns, rows 1 .. m inside a strip
  int32_t score = (m == 0 && n == 0) ? 0 : NEG;            // M[m][0] = M[0][n] = NEG (:225, :231)
  if (m > 0 && n > 0) {
    const int nstrips = (n + AL_STRIP - 1) / AL_STRIP;
    for (int s = 0; s < nstrips; ++s) {
      const int c0 = s * AL_STRIP;                          // 0-based index of the strip's first column (column c0 + 1)
      uint32_t boff[AL_STRIP];
      int32_t MG[AL_STRIP], X[AL_STRIP];
#pragma unroll
      for (int c = 0; c < AL_STRIP; ++c) {
        const int col = c0 + c;
        boff[c] = (col < n ? (uint32_t)s2[col] : 0u) * (uint32_t)sizeof(int32_t);
        MG[c] = max(NEG, -go - col * ge) - goe;             // max(M,Ix,Iy)[0][col+1] - goe = Iy[0][col+1] - goe
        X[c] = NEG;
      }
      int32_t mg_prev = c0 == 0 ? -goe : (max(NEG, -go - (c0 - 1) * ge) - goe);   // best[0][c0] - goe: the diagonal neighbour of row 1
      const bool more = s + 1 < nstrips;
      for (int r = 1; r <= m; ++r) {
        const uint32_t a = s1[r - 1];
        const char *tab_row = tab_bytes + a * (24u * (uint32_t)sizeof(int32_t));
        int32_t *brow = bnd + (size_t)(r - 1) * 2 * 64;
        int32_t mg_in = NEG - goe, y_in = NEG;              // column 0: M[r][0] = Iy[r][0] = NEG (:224-229)
        if (s > 0) { mg_in = brow[0]; y_in = brow[64]; }    // the last column of the strip to the left
        uint32_t w0, w1;
        int32_t y_out;
        if (r == 1) al_row<true>(MG, X, boff, tab_row, mg_prev, mg_in, y_in, ge, goe, ix_first, w0, w1, y_out);
        else al_row<false>(MG, X, boff, tab_row, mg_prev, mg_in, y_in, ge, goe, ix_first, w0, w1, y_out);
        mg_prev = s == 0 ? (max(NEG, -go - (r - 1) * ge) - goe) : mg_in;   // best[r][c0] - goe; column 0: Ix[r][0]
        uint32_t *drow = dec + ((size_t)(r - 1) * AL_WORDS + 2 * s) * 64;
        drow[0] = w0;
        drow[64] = w1;
        if (more) { brow[0] = MG[AL_STRIP - 1]; brow[64] = y_out; }
      }
      if (!more) {
        const int own = (n - 1) - c0;
#pragma unroll
        for (int c = 0; c < AL_STRIP; ++c)
          if (c == own) score = MG[c] + goe;
      }
    }
  }
  bnd[AL_SCORE_SLOT] = score;
}

// the back walk (reference :284-308) over the words k_nw_align_fill left for this lane
__global__ __launch_bounds__(AL_THREADS) void k_nw_align_walk(const uint8_t *__restrict__ x_codes, const int64_t *__restrict__ x_off, int64_t m_seqs,
                                                              const uint8_t *__restrict__ y_codes, const int64_t *__restrict__ y_off, int64_t n_seqs,
                                                              const int32_t *__restrict__ pair_x, const int32_t *__restrict__ pair_y,
                                                              int64_t pair_base, int64_t pairs, uint8_t *__restrict__ ops_out, int64_t ld_ops,
                                                              int32_t *__restrict__ len_out, int32_t *__restrict__ matches_out,
                                                              int32_t *__restrict__ score_out, uint32_t *work) {
  const int64_t q = (int64_t)blockIdx.x * AL_THREADS + threadIdx.x;
  if (q >= pairs) return;
  const AlignPair pr = al_pair(x_codes, x_off, m_seqs, y_codes, y_off, n_seqs, pair_x, pair_y, pair_base, q, ops_out != nullptr, ld_ops);
  if (!pr.ok) {
    if (len_out) len_out[q] = -1;
    if (matches_out) matches_out[q] = -1;
    if (score_out) score_out[q] = 0;
    return;
  }
  const uint32_t *dec = al_dec(work, q);
  const int m = pr.m, n = pr.n;
  const uint8_t *s1 = pr.s1, *s2 = pr.s2;
  auto step = [&](int i, int j) -> uint32_t {
    if (i == 0) return 2u;                                  // (0, j): L
    if (j == 0) return 1u;                                  // (i, 0): U
    const uint32_t w = dec[((size_t)(i - 1) * AL_WORDS + ((j - 1) >> 4)) * 64];
    return (w >> (2 * ((j - 1) & 15))) & 3u;
  };
  int i = m, j = n, len = 0, mt = 0;
  while (i > 0 || j > 0) {
    const uint32_t code = step(i, j);
    if (code == 0u) { mt += s1[i - 1] == s2[j - 1]; --i; --j; }
    else if (code == 1u) --i;
    else --j;
    ++len;
  }
  if (len_out) len_out[q] = len;
  if (matches_out) matches_out[q] = mt;
  if (score_out) score_out[q] = al_bnd(work, q)[AL_SCORE_SLOT];
  if (ops_out) {                                            // forward order: filled from the back; bytes past len stay 0 (the launcher cleared them)
    uint8_t *ops = ops_out + (size_t)q * (size_t)ld_ops;
    i = m; j = n;
    int pos = len;
    while (i > 0 || j > 0) {
      const uint32_t code = step(i, j);
      ops[--pos] = code == 0u ? (uint8_t)'D' : (code == 1u ? (uint8_t)'U' : (uint8_t)'L');
      if (code == 0u) { --i; --j; }
      else if (code == 1u) --i;
      else --j;
    }
  }
}

}  // namespace

size_t nw_align_workspace_bytes(int64_t pairs) { return pairs <= 0 ? 0 : (size_t)ceil_div(pairs, 64) * AL_WAVE_BYTES; }

// `pairs` pairs starting at entry pair_base of the lists (outputs likewise), in launches of as many pairs as the workspace holds: launches on
// one stream run in order, so they share it.
int launch_nw_align(const uint8_t *d_x_codes, const int64_t *d_x_off, int64_t m, const uint8_t *d_y_codes, const int64_t *d_y_off, int64_t n,
                    const int32_t *d_pair_x, const int32_t *d_pair_y, int64_t pair_base, int64_t pairs, int matrix_id, int gap_open, int gap_ext,
                    uint8_t *d_ops, int64_t ld_ops, int32_t *d_len, int32_t *d_matches, int32_t *d_score, void *d_work, size_t work_bytes,
                    hipStream_t stream) {
  if (pairs <= 0) return DA_OK;
  const signed char *tab = matrix_table_host(matrix_id);
  if (!tab) return fail(DA_ERR_BAD_ARG, "matrix id %d out of range", matrix_id);
  const int64_t waves = (int64_t)(work_bytes / AL_WAVE_BYTES);
  if (!d_work || waves < 1)
    return fail(DA_ERR_BAD_ARG, "the alignment workspace holds less than one wavefront of pairs (%zu bytes; da_nw_align_workspace_bytes)", work_bytes);
  AlignTable st;
  for (int e = 0; e < 576; ++e) st.s[e] = tab[e];
  if (d_ops) DA_HIP_TRY(hipMemsetAsync(d_ops, 0, (size_t)pairs * (size_t)ld_ops, stream));
  const int64_t step = std::min<int64_t>(waves * 64, (int64_t)1 << 30);
  for (int64_t p0 = 0; p0 < pairs; p0 += step) {
    const int64_t cnt = std::min(step, pairs - p0);
    const dim3 grid((unsigned)ceil_div(cnt, AL_THREADS)), block(AL_THREADS);
    const int32_t *lx = d_pair_x ? d_pair_x + p0 : nullptr, *ly = d_pair_y ? d_pair_y + p0 : nullptr;
    hipLaunchKernelGGL(k_nw_align_fill, grid, block, 0, stream, d_x_codes, d_x_off, m, d_y_codes, d_y_off, n, lx, ly, pair_base + p0, cnt, st,
                       (int32_t)gap_open, (int32_t)gap_ext, d_ops != nullptr, ld_ops, static_cast<uint32_t *>(d_work));
    hipLaunchKernelGGL(k_nw_align_walk, grid, block, 0, stream, d_x_codes, d_x_off, m, d_y_codes, d_y_off, n, lx, ly, pair_base + p0, cnt,
                       d_ops ? d_ops + (size_t)p0 * (size_t)ld_ops : nullptr, ld_ops, d_len ? d_len + p0 : nullptr,
                       d_matches ? d_matches + p0 : nullptr, d_score ? d_score + p0 : nullptr, static_cast<uint32_t *>(d_work));
    DA_HIP_TRY(hipGetLastError());
  }
  return DA_OK;
}

}  // namespace da
