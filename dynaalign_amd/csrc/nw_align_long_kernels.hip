// nw_align_long_kernels.hip -- the alignment PATH of listed pairs of up to 1024 residues a side (da_nw_align_long_pairs,
// da_dev_nw_align_long_pairs).
//
// nw_align_kernels.hip keeps both sequences of a pair in one lane and stops at 127 residues.  Here ONE WAVEFRONT takes a pair:
//   * the fill is the anti-diagonal sweep of k_nw_long (nw_kernels.hip): lane l owns W consecutive columns of sequence2 and works on
//     row t - l + 1 at step t; the last column's (best - goe, Iy, payload) goes one lane up per step; sequence1 and the score table sit
//     in LDS.  The cell is the int32 three-state cell of nw_row() with its (matches << 16 | length) payload, same boundaries, same
//     tie-break: length, matches and M[m][n] come out of the fill exactly as in K4.
//   * W is chosen per pair among the widths K4 is built for (1, 2, 3, 4, 6, 8, 9, 12, 16): the smallest with 64 W >= len(sequence2).
//     The switch is wave-uniform.
//   * with ops wanted, the row function also packs the decision of each of its W cells (0 D, 1 U, 2 L; 2 bits) into one word, stored
//     [step][lane]: the wave's store of a step is 256 consecutive bytes.  A pair of m rows needs (m + 63) * 256 bytes: a SLOT is
//     (max_len + 63) * 256 bytes.  The grid is persistent: wave s takes pairs s, s + slots, ... and reuses slot s.
//   * the same wave then walks the pair back (reference src/pairwiseSeqAlign.cpp:284-308).  Cell (i, j) lives in lane (j - 1) / W at
//     step i - 1 + lane, and that step never increases along the walk, so the walk slides a window of ALL_CHUNK consecutive steps
//     through LDS: each lane loads the words it stored itself (coalesced, program order suffices), the walk is wave-uniform and reads
//     one LDS word per move.  The ops bytes are written from the back, 64 at a time: lane p & 63 holds the byte of position p.
//   * without ops: no decision word, no walk, no workspace; the three integers come from the payload.
#include <algorithm>
#include <climits>

#include "da_common.hpp"

namespace da {

const signed char *matrix_table_host(int id);   // nw_kernels.hip

namespace {

struct LongTable { signed char s[576]; };   // passed by value in the kernarg segment
struct LCell { int32_t s_goe; uint32_t inc; };   // LDS table entry: score + goe, 1 + (a == b) << 16

constexpr int ALL_THREADS = 256;
constexpr int ALL_WAVES = ALL_THREADS / 64;
constexpr int ALL_MAXLEN = 1024;                 // 64 lanes x W <= 16 columns
constexpr int ALL_CHUNK = 32;                    // steps in the walk's window: 8 KiB of LDS per wave
constexpr int64_t ALL_SLOT_CAP = 3072;           // resident waves worth a slot: 256 CUs x 3 workgroups (LDS, registers) x 4 waves
constexpr int64_t ALL_WAVES_NO_OPS = 4096;       // without the window: 4 workgroups per CU (max_len <= 576)
constexpr size_t all_slot_words(int64_t max_len) { return (size_t)(max_len + 63) * 64; }

// One DP row for a lane, its W columns left to right: nw_row() of nw_kernels.hip, which already computes the two booleans that ARE the
// decision.  DEC: also pack them, cell w at bits 2 w of the returned word.
template <int W, bool FIRST, bool DEC>
__device__ __forceinline__ uint32_t all_row(int32_t (&MG)[W], int32_t (&X)[W], uint32_t (&P)[W], const uint32_t (&boff)[W], const char *tab_row,
                                            int32_t mgd, uint32_t pd, uint32_t pl, int32_t mgl, int32_t yl, int32_t ge, int32_t goe,
                                            int32_t ix_first, int32_t &y_last) {
  uint32_t word = 0u;
#pragma unroll
  for (int c = 0; c < W; ++c) {
    const LCell e = *reinterpret_cast<const LCell *>(tab_row + boff[c]);
    const int32_t ix = FIRST ? ix_first : max(MG[c], X[c] - ge);          // reference :255-257
    const int32_t iy = max(mgl, yl - ge);                                   // :260-262
    const int32_t d = mgd + e.s_goe;                                        // :265-268
    const int32_t gap = max(ix, iy);
    const bool take_d = d >= gap;                                           // :271
    const bool up_over_left = ix >= iy;                                     // :273
    const int32_t m = max(d, gap);                                          // :272-278 (M overwrite)
    const uint32_t p_gap = (up_over_left ? P[c] : pl) + 1u;
    const uint32_t p_new = take_d ? pd + e.inc : p_gap;
    if (DEC) word |= (take_d ? 0u : (up_over_left ? 1u : 2u)) << (2 * c);
    mgd = MG[c];
    pd = P[c];
    mgl = m - goe;
    yl = iy;
    pl = p_new;
    MG[c] = mgl;
    X[c] = ix;
    P[c] = p_new;
  }
  y_last = yl;
  return word;
}

// The fill of one pair (m, nn >= 1) by one wave: the sweep of nw_long_body.  dec (DEC only): the wave's slot, [step][lane].
template <int W, bool DEC>
__device__ __forceinline__ void all_fill(const uint8_t *__restrict__ s2, int nn, int m, const uint8_t *s1, const char *tab_bytes, int32_t go,
                                         int32_t ge, uint32_t *dec, int lane_in, uint32_t &p_res, int32_t &sc_res) {
  int lane = lane_in;
  asm volatile("" : "+v"(lane));            // every width starts from its own copy: nothing of one case is computed ahead of the switch
  const int32_t goe = go + ge;
  const int32_t NEG = INT_MIN / 2;
  const int32_t ix_first = max(NEG - goe, NEG - ge);
  const int la = (nn + W - 1) / W;          // lanes that own at least one real column
  const int c_first = lane * W;             // 0-based index of this lane's first column
  uint32_t boff[W];
  int32_t MG[W], X[W];
  uint32_t P[W];
#pragma unroll
  for (int w = 0; w < W; ++w) {
    const int c = c_first + w;              // column c + 1
    boff[w] = (c < nn ? (uint32_t)s2[c] : 0u) * (uint32_t)sizeof(LCell);
    MG[w] = max(NEG, -go - c * ge) - goe;   // max(M,Ix,Iy)[0][c+1] - goe
    X[w] = NEG;
    P[w] = (uint32_t)(c + 1);
  }
  int32_t mg_prev = (lane == 0) ? -goe : (max(NEG, -go - (c_first - 1) * ge) - goe);  // max(M,Ix,Iy)[0][c_first] - goe
  uint32_t p_prev = (uint32_t)c_first;
  int32_t mg_send = 0, y_send = 0;
  uint32_t p_send = 0;
  const int own_lane = (nn - 1) / W, own_w = (nn - 1) - own_lane * W;
  const int steps = m + la - 1;
  for (int t = 0; t < steps; ++t) {
    int32_t mg_in = __shfl_up(mg_send, 1);
    int32_t y_in = __shfl_up(y_send, 1);
    uint32_t p_in = (uint32_t)__shfl_up((int)p_send, 1);
    const int r = t - lane + 1;             // DP row of this lane in this step
    if (lane == 0) { mg_in = NEG - goe; y_in = NEG; p_in = (uint32_t)r; }
    if (lane < la && r >= 1 && r <= m) {
      const uint32_t a = s1[r - 1];
      const char *tab_row = tab_bytes + a * (24u * (uint32_t)sizeof(LCell));
      int32_t y_out;
      uint32_t word;
      if (r == 1)
        word = all_row<W, true, DEC>(MG, X, P, boff, tab_row, mg_prev, p_prev, p_in, mg_in, y_in, ge, goe, ix_first, y_out);
      else
        word = all_row<W, false, DEC>(MG, X, P, boff, tab_row, mg_prev, p_prev, p_in, mg_in, y_in, ge, goe, ix_first, y_out);
      if (DEC) dec[(size_t)t * 64 + lane] = word;                             // t < m + 63 <= max_len + 63: inside the slot
      mg_prev = (lane == 0) ? (max(NEG, -go - (r - 1) * ge) - goe) : mg_in;   // lane 0: max(M,Ix,Iy)[r][0] = Ix[r][0]
      p_prev = p_in;
      mg_send = MG[W - 1];
      y_send = y_out;
      p_send = P[W - 1];
      if (r == m && lane == own_lane) {
#pragma unroll
        for (int w = 0; w < W; ++w)
          if (w == own_w) { p_res = P[w]; sc_res = MG[w] + goe; }
      }
    }
  }
  p_res = (uint32_t)__shfl((int)p_res, own_lane);
  sc_res = __shfl(sc_res, own_lane);
}

// The back walk of one pair (m, nn >= 1) from (m, nn), wave-uniform.  win: the wave's window of ALL_CHUNK steps.  ops[0 .. len) is filled from the
// back; lane p & 63 keeps the byte of position p until its group of 64 is complete.
__device__ __forceinline__ void all_walk(int m, int nn, int W, const uint32_t *dec, uint32_t *win, uint8_t *__restrict__ ops, int len,
                                         int lane) {
  int i = m, j = nn, pos = len;
  int l = (nn - 1) / W, w = (nn - 1) - l * W;   // lane and column-in-lane of column j (j >= 1)
  int t_lo = INT_MAX;                            // first step in the window: nothing loaded yet
  uint32_t mine = 0u;
  while ((i > 0 || j > 0) && pos > 0) {
    uint32_t code;
    if (i == 0) code = 2u;                       // (0, j): L
    else if (j == 0) code = 1u;                  // (i, 0): U
    else {
      const int t = i - 1 + l;
      if (t < t_lo) {                            // the chunk below: steps t_lo .. t of the slot, each lane its own words
        __builtin_amdgcn_wave_barrier();
        t_lo = max(0, t + 1 - ALL_CHUNK);
#pragma unroll 8
        for (int s = 0; s < ALL_CHUNK; ++s) {
          const int ts = t_lo + s;
          win[s * 64 + lane] = ts <= t ? dec[(size_t)ts * 64 + lane] : 0u;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
      const uint32_t word = (uint32_t)__builtin_amdgcn_readfirstlane((int)win[(t - t_lo) * 64 + l]);
      code = (word >> (2 * w)) & 3u;
    }
    --pos;
    if (lane == (pos & 63)) mine = code == 0u ? (uint32_t)'D' : (code == 1u ? (uint32_t)'U' : (uint32_t)'L');
    if ((pos & 63) == 0 && pos + lane < len) ops[pos + lane] = (uint8_t)mine;
    if (code != 2u) --i;
    if (code != 1u) {
      --j;
      if (--w < 0) { w = W - 1; --l; }
    }
  }
}

// pair q: x[pair_x[q]] (sequence1) against y[pair_y[q]] (sequence2); pair_x == NULL: both indices are pair_base + q.  Persistent: wave s of
// `waves` takes pairs s, s + waves, ...; with ops it owns slot s of the workspace.
// WMAX: the widest W this instance holds (4, 9 or 16): the launcher picks it from max_len, so a launch of HA-sized sequences is not held to the
// registers of W = 16.
template <bool DEC, int WMAX>
__global__ __launch_bounds__(ALL_THREADS) __attribute__((amdgpu_waves_per_eu(WMAX > 9 ? 2 : 3))) void k_nw_align_long(const uint8_t *__restrict__ x_codes, const int64_t *__restrict__ x_off, int64_t m_seqs,
                                                               const uint8_t *__restrict__ y_codes, const int64_t *__restrict__ y_off, int64_t n_seqs,
                                                               const int32_t *__restrict__ pair_x, const int32_t *__restrict__ pair_y,
                                                               int64_t pair_base, int64_t pairs, LongTable table, int32_t go, int32_t ge,
                                                               int32_t max_len, uint8_t *__restrict__ ops_out, int64_t ld_ops,
                                                               int32_t *__restrict__ len_out, int32_t *__restrict__ matches_out,
                                                               int32_t *__restrict__ score_out, uint32_t *work, int64_t waves) {
  __shared__ __attribute__((aligned(16))) LCell tab[24 * 24];
  __shared__ uint8_t seq1[ALL_WAVES][ALL_MAXLEN];
  __shared__ uint32_t window[DEC ? ALL_WAVES : 1][DEC ? ALL_CHUNK * 64 : 1];
  const int32_t goe = go + ge;
  for (int e = threadIdx.x; e < 576; e += ALL_THREADS) {
    const int a = e / 24, b = e - a * 24;
    tab[e].s_goe = (int32_t)table.s[e] + goe;
    tab[e].inc = 1u + ((a == b) ? 0x10000u : 0u);
  }
  __syncthreads();
  const char *tab_bytes = reinterpret_cast<const char *>(tab);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;   // wave-uniform: pair data in scalars
  const int64_t slot = (int64_t)blockIdx.x * ALL_WAVES + wave;
  if (slot >= waves) return;                               // no barrier below: a wave may leave
  uint8_t *s1 = seq1[wave];
  uint32_t *win = window[DEC ? wave : 0];
  uint32_t *dec = DEC ? work + (size_t)slot * all_slot_words(max_len) : nullptr;
  const int32_t NEG = INT_MIN / 2;

  for (int64_t q = slot; q < pairs; q += waves) {
    const int64_t ix = pair_x ? (int64_t)pair_x[q] : pair_base + q;
    const int64_t iy = pair_y ? (int64_t)pair_y[q] : pair_base + q;
    bool ok = ix >= 0 && ix < m_seqs && iy >= 0 && iy < n_seqs;
    int64_t b1 = 0, b2 = 0, l1 = 0, l2 = 0;
    if (ok) {
      b1 = x_off[ix]; l1 = x_off[ix + 1] - b1; b2 = y_off[iy]; l2 = y_off[iy + 1] - b2;
      ok = l1 >= 0 && l1 <= max_len && l2 >= 0 && l2 <= max_len && (!DEC || l1 + l2 <= ld_ops);
    }
    if (!ok) {   // a pair the kernel cannot take: the host call has refused it before, the device-pointer call reports it this way
      if (lane == 0) {
        if (len_out) len_out[q] = -1;
        if (matches_out) matches_out[q] = -1;
        if (score_out) score_out[q] = 0;
      }
      continue;
    }
    const int m = __builtin_amdgcn_readfirstlane((int)l1), nn = __builtin_amdgcn_readfirstlane((int)l2);
    uint8_t *ops = DEC ? ops_out + (size_t)q * (size_t)ld_ops : nullptr;
    uint32_t p_res = 0;       // matches << 16 | length of cell (m, nn)
    int32_t sc_res = NEG;
    int W = 16;
    if (m == 0 || nn == 0) {  // boundary cells (reference :222-235): an all-L or all-U path
      p_res = (uint32_t)(m == 0 ? nn : m);
      sc_res = (m == 0 && nn == 0) ? 0 : NEG;
      if (DEC)
        for (int p = lane; p < (int)p_res; p += 64) ops[p] = m == 0 ? (uint8_t)'L' : (uint8_t)'U';
    } else {
      for (int p = lane; p < m; p += 64) s1[p] = x_codes[b1 + p];   // same wave reads it back: program order suffices
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const uint8_t *s2 = y_codes + b2;
      W = nn <= 64 ? 1 : nn <= 128 ? 2 : nn <= 192 ? 3 : nn <= 256 ? 4 : nn <= 384 ? 6 : nn <= 512 ? 8 : nn <= 576 ? 9 : nn <= 768 ? 12 : 16;
      switch (W) {
#define ALL_CASE(WW) case WW: if constexpr (WW < WMAX) { all_fill<WW, DEC>(s2, nn, m, s1, tab_bytes, go, ge, dec, lane, p_res, sc_res); break; }
        ALL_CASE(1) ALL_CASE(2) ALL_CASE(3) ALL_CASE(4) ALL_CASE(6) ALL_CASE(8) ALL_CASE(9) ALL_CASE(12)
        default: all_fill<WMAX, DEC>(s2, nn, m, s1, tab_bytes, go, ge, dec, lane, p_res, sc_res); break;   // max_len <= 64 WMAX: W == WMAX here
#undef ALL_CASE
      }
      if (DEC) all_walk(m, nn, W, dec, win, ops, (int)(p_res & 0xffffu), lane);
      __builtin_amdgcn_wave_barrier();   // the next pair overwrites s1
    }
    if (lane == 0) {
      if (len_out) len_out[q] = (int32_t)(p_res & 0xffffu);
      if (matches_out) matches_out[q] = (int32_t)(p_res >> 16);
      if (score_out) score_out[q] = sc_res;
    }
  }
}

}  // namespace

size_t nw_align_long_slot_bytes(int64_t max_len) { return all_slot_words(std::min<int64_t>(std::max<int64_t>(max_len, 0), ALL_MAXLEN)) * sizeof(uint32_t); }

size_t nw_align_long_workspace_bytes(int64_t pairs, int64_t max_len) {
  if (pairs <= 0 || max_len < 0) return 0;
  return (size_t)std::min(pairs, ALL_SLOT_CAP) * nw_align_long_slot_bytes(max_len);
}

// `pairs` pairs starting at entry pair_base of the lists (outputs likewise) in ONE persistent launch of as many waves as the workspace has
// slots (at most ALL_SLOT_CAP); without d_ops no workspace is read and ALL_WAVES_NO_OPS waves run.
int launch_nw_align_long(const uint8_t *d_x_codes, const int64_t *d_x_off, int64_t m, const uint8_t *d_y_codes, const int64_t *d_y_off, int64_t n,
                         const int32_t *d_pair_x, const int32_t *d_pair_y, int64_t pair_base, int64_t pairs, int matrix_id, int gap_open, int gap_ext,
                         uint8_t *d_ops, int64_t ld_ops, int32_t *d_len, int32_t *d_matches, int32_t *d_score, int64_t max_len, void *d_work,
                         size_t work_bytes, hipStream_t stream) {
  if (pairs <= 0) return DA_OK;
  const signed char *tab = matrix_table_host(matrix_id);
  if (!tab) return fail(DA_ERR_BAD_ARG, "matrix id %d out of range", matrix_id);
  if (max_len < 0) return fail(DA_ERR_BAD_ARG, "negative max_len");
  const int32_t ml = (int32_t)std::min<int64_t>(max_len, ALL_MAXLEN);
  int64_t waves = std::min(pairs, d_ops || ml > 576 ? ALL_SLOT_CAP : ALL_WAVES_NO_OPS);   // the W = 16 instance holds 3 waves per SIMD without ops too
  if (d_ops) {
    const int64_t slots = d_work ? (int64_t)(work_bytes / nw_align_long_slot_bytes(ml)) : 0;
    if (slots < 1)
      return fail(DA_ERR_BAD_ARG, "the alignment workspace holds less than one slot of (max_len + 63) * 256 bytes (%zu bytes; da_nw_align_long_workspace_bytes)",
                  work_bytes);
    waves = std::min(waves, slots);
  }
  LongTable st;
  for (int e = 0; e < 576; ++e) st.s[e] = tab[e];
  if (d_ops) DA_HIP_TRY(hipMemsetAsync(d_ops, 0, (size_t)pairs * (size_t)ld_ops, stream));
  const dim3 grid((unsigned)ceil_div(waves, ALL_WAVES)), block(ALL_THREADS);
  uint8_t *ops = d_ops;
  uint32_t *work = d_ops ? static_cast<uint32_t *>(d_work) : nullptr;
#define ALL_LAUNCH(DEC, WMAX)                                                                                                                       \
  hipLaunchKernelGGL((k_nw_align_long<DEC, WMAX>), grid, block, 0, stream, d_x_codes, d_x_off, m, d_y_codes, d_y_off, n, d_pair_x, d_pair_y, pair_base, \
                     pairs, st, (int32_t)gap_open, (int32_t)gap_ext, ml, ops, ld_ops, d_len, d_matches, d_score, work, waves)
  if (ml <= 256) { if (d_ops) ALL_LAUNCH(true, 4); else ALL_LAUNCH(false, 4); }
  else if (ml <= 576) { if (d_ops) ALL_LAUNCH(true, 9); else ALL_LAUNCH(false, 9); }
  else { if (d_ops) ALL_LAUNCH(true, 16); else ALL_LAUNCH(false, 16); }
#undef ALL_LAUNCH
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

}  // namespace da
