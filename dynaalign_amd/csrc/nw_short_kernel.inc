// nw_short_kernel.inc -- the text of K3, included twice by nw_kernels.hip: as k_nw_short (NW_SHORT_COLS false: every mode the kernel had, the
// column arguments are not read) and as k_nw_short_cols (true: the row-block mode restricted to the columns [col_begin, col_end), da_dev_nw_rect).
// Why an include file and not one of the two tidier shapes (both built and compared with `make resources` against the kernels as they were):
//   * a sixth template parameter COLS on k_nw_short compiled every existing instantiation to the same VGPRs, SGPRs, scratch and occupancy,
//     but renamed them all ("k_nw_short<20, true, true, false, true, false>"): bench.py looks the kernel up by name in the PMC summaries;
//   * a __device__ __forceinline__ body behind two thin __global__ wrappers (what K4 / K5 do) kept the names but not the allocation:
//     k_nw_short<16, true, true, false, true> went from 75 to 87 VGPRs (6 -> 5 waves per SIMD), <16, true, true> 71 -> 72, ten more
//     instantiations +2 SGPRs, <32, true, *> 3 VGPRs fewer -- presumably because __restrict__ on an inlined function's parameters is
//     weaker than on a kernel's.  Worth retrying with a newer compiler; the text below needs only its first lines changed back.
// k_nw_short therefore carries the two column arguments without reading them (NW_SHORT_COLS false makes them constants).
template <int NMAX, bool CK, bool ORD, bool ASM = false, bool PFX = false>
__global__ __launch_bounds__(K3_THREADS, (NMAX <= 24 ? (CK && ORD && !ASM ? 5 : 4) : 1)) void NW_SHORT_NAME(   // <= 24 residues: 4 waves per SIMD (128 VGPRs); the ordered mode FIVE (96 VGPRs; PFX: 30 KB of LDS) since its table offsets are packed (round 4b; the direct sweep: 422 ms that way, 404 at four)
    const uint8_t *__restrict__ codes, const int64_t *__restrict__ offsets, int64_t n,
    ScoreTable table, int32_t go, int32_t ge, int64_t row_begin, int64_t row_end, int symmetric,
    int kind, void *__restrict__ out_v, int64_t ld, int32_t *__restrict__ score_out,
    int64_t ld_score, int64_t ntiles, int T, int shard_rank, int shard_world, int fold_q, int64_t fold_w,
    const int32_t *__restrict__ ord_first, const int32_t *__restrict__ ord_minfirst, const int32_t *__restrict__ ord_maxlast,
    const int32_t *__restrict__ ord_perm, const uint8_t *__restrict__ ord_lcp, int64_t col_begin_arg, int64_t col_end_arg) {
  // [col_begin, col_end): the columns of a row-block request (COLS, da_dev_nw_rect; T = its 64-column tile columns); [0, n) in every other mode
  constexpr bool COLS = NW_SHORT_COLS;
  const int64_t col_begin = COLS ? col_begin_arg : 0, col_end = COLS ? col_end_arg : n;
  // ord_first != NULL: ORDERED mode on a table of UNIQUE sequences (nw_dedup below): element (p, q) of the full square is
  // calc(U_p, U_q) with U_p as sequence1 whatever the order of p and q, computed only where some pair i < j of the original
  // input maps to it: first(p) < last(q) (or p == q).
  constexpr bool ordered = ORD;               // (a template parameter: the two modes show up as two kernels in profiles)
  const bool f64_out = kind == DA_OUT_F64;
  __shared__ __attribute__((aligned(16))) Cell tab[CK ? 1 : 24 * 24];
  __shared__ int32_t tabk[CK ? 24 * 24 : 1];
  __shared__ uint8_t rowcodes[K3_TILE][NMAX];
  __shared__ int32_t rowlen[K3_TILE];
  __shared__ int32_t rowid[PFX ? K3_TILE : 1];      // PFX: unique id of the row at this sorted position (-1 past the end)
  __shared__ uint8_t rowlcp[PFX ? K3_TILE : 1];     // ... its common prefix with the previous sorted row (0 at a wave's first row)
  __shared__ uint8_t rowneed[PFX ? K3_TILE : 1];    // ... whether this tile needs the row at all
  __shared__ uint32_t mirror_res[ORD ? 1 : K3_THREADS / 64][ORD ? 1 : K3_ROWS_PER_WAVE][64];   // (ordered mode never mirrors)
  // PFX: a lane's checkpoint lives in LDS, [word][thread]: NMAX words of VM + NMAX / 2 words of Ix' scores packed two by two (the rest of an
  // XP word is priority 1 + the payload of the same column's VM) -- 30 KB at NMAX = 20, four workgroups per CU, no extra VGPRs
  // round 4b: the Ix' part as BYTES: d = score(VM[c]) - score(XP[c]) is >= 0 (VM is the max of three that include Ix') and only matters up to `go` --
  // the next row takes max(VM[c] + kx, XP[c]) with score(VM[c] + kx) = score(VM[c]) - go, same priority, same payload: at d >= go the first operand wins or
  // ties bit for bit -- so min(d, go) <= 255 is stored, four columns per word: 25 words = 25.6 KB at NMAX = 20, FIVE workgroups per CU
  static_assert(!PFX || NMAX % 4 == 0, "the checkpoint packs four columns per word");
  __shared__ uint32_t cp_lds[PFX ? NMAX + NMAX / 4 : 1][PFX ? K3_THREADS : 1];

  // ---- tile decode (upper-triangular 64x64 tiles of the pair space)
  const int64_t L = blockIdx.x;
  if (L >= ntiles) return;
  int ti, tj;
  bool allow_direct = true, allow_mirror = true;
  int64_t row_shift = -row_begin;  // local output row = global row + row_shift
  int64_t col_shift = -col_begin;  // local output column = global column + col_shift (direct stores)
  if (ordered) {
    ti = (int)(row_begin / K3_TILE) + (int)(L / T);              // (row_begin, row_end: whole 64-row tile rows of the unique table)
    tj = (int)(L % T);
    if (shard_world > 0) {     // one rank's cyclic 128-row units of the ordered table, stored back to back: local unit u = global unit u * world + rank
      const int q64 = (int)(L / T), u = q64 >> 1;
      ti = 2 * (u * shard_world + shard_rank) + (q64 & 1);
      if (ti >= T) return;
      row_shift = (int64_t)u * 128 + (int64_t)(q64 & 1) * K3_TILE - (int64_t)ti * K3_TILE;
    }
    if (!PFX && ti != tj && ord_minfirst[ti] >= ord_maxlast[tj]) return;   // no original pair i < j needs this tile (PFX: rows are in sorted order, decided per row)
    allow_mirror = false;
  } else if (symmetric) {
    // row-major over the upper triangle: row t holds T - t tiles
    const double Td = (double)T;
    int64_t t = (int64_t)(Td + 0.5 - sqrt((Td + 0.5) * (Td + 0.5) - 2.0 * (double)L));
    if (t < 0) t = 0;
    if (t > T - 1) t = T - 1;
    auto start = [&](int64_t r) { return r * T - r * (r - 1) / 2; };
    while (t > 0 && start(t) > L) --t;
    while (t + 1 <= T - 1 && start(t + 1) <= L) ++t;
    ti = (int)t;
    tj = (int)(t + (L - start(t)));
  } else if (shard_world > 0) {
    // cyclic shard of one rank: local unit u is global 128-row unit u*world + rank; only
    // upper tiles, direct store into local rows q*64 + [0,64) (the mirror is filled after
    // the all-gather by k_finalize_sharded)
    // ranks are dealt 128-row UNITS (two of this kernel's 64-row tile rows), the same unit and folded layout as the
    // MinHash shards -- so the histogram / edge-extraction kernels (graph_kernels.hip) read both kinds of block
    const int q64 = (int)(L / T);                         // local 64-row tile row
    const int u = q64 >> 1;                               // local unit
    const int gu = u * shard_world + shard_rank;          // global unit
    ti = 2 * gu + (q64 & 1);
    tj = (int)(L % T);
    if (ti >= T || tj < ti) return;
    allow_mirror = false;
    {  // folded shard layout (ShardGeom, tile = 128): units u and Q-1-u share a stored unit row
      const bool front = u <= fold_q - 1 - u;
      row_shift = (int64_t)(front ? u : fold_q - 1 - u) * 128 + (int64_t)(q64 & 1) * K3_TILE - (int64_t)ti * K3_TILE;
      col_shift = front ? -(int64_t)gu * 128 : shard_back(fold_w, n);
    }
  } else {
    // row-block request: tile row rt (inside the block) x every tile column tc.
    // tc >= rt is the upper tile itself (direct store); tc < rt is served by
    // the upper tile (tc, rt) through its mirrored store, so each element of
    // the block is produced exactly once.
    const int rt = (int)(row_begin / K3_TILE) + (int)(L / T);
    const int tc = (int)(col_begin / K3_TILE) + (int)(L % T);
    ti = tc >= rt ? rt : tc;
    tj = tc >= rt ? tc : rt;
    allow_direct = tc >= rt;
    allow_mirror = tc <= rt;
  }
  const int64_t I0 = (int64_t)ti * K3_TILE, J0 = (int64_t)tj * K3_TILE;
  const int32_t goe = go + ge;
  const int32_t NEG = INT_MIN / 2;

  // ---- stage the score table and this tile's 64 row sequences in LDS
  for (int e = threadIdx.x; e < 576; e += K3_THREADS) {
    const int a = e / 24, b = e - a * 24;
    if (CK) {
      tabk[e] = (((int32_t)table.s[e] + 2 * ge) << CKBits<NMAX>::S2) + (2 << CKBits<NMAX>::S) + 1 + ((a == b) ? (1 << CKBits<NMAX>::LB) : 0);
    } else {
      tab[e].s_goe = (int32_t)table.s[e] + goe;
      tab[e].inc = 1u + ((a == b) ? 0x10000u : 0u);  // equal index <=> equal residue byte (:291-293)
    }
  }
  for (int r = threadIdx.x >> 2; r < K3_TILE; r += K3_THREADS / 4) {
    int64_t i = I0 + r;
    if (PFX) {
      const int64_t pos = i;
      i = pos < n ? (int64_t)ord_perm[pos] : n;                    // the row's unique id
      if ((threadIdx.x & 3) == 0) {
        rowid[r] = pos < n ? (int32_t)i : -1;
        rowlcp[r] = (pos < n && r != 0) ? ord_lcp[pos] : (uint8_t)0;
        rowneed[r] = (pos < n && ((int)(i / K3_TILE) == tj || ord_first[i] < ord_maxlast[tj])) ? (uint8_t)1 : (uint8_t)0;
      }
    }
    const int64_t b = i < n ? offsets[i] : 0;
    const int32_t len = i < n ? (int32_t)(offsets[i + 1] - b) : 0;
    if ((threadIdx.x & 3) == 0) rowlen[r] = len;
    for (int q = threadIdx.x & 3; q < NMAX; q += 4) rowcodes[r][q] = q < len ? codes[b + q] : 0;
  }

  // ---- lane-private sequence2
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t j = J0 + lane;
  const bool jvalid = j < n;
  int32_t nj = 0;
  uint32_t boff[NMAX];
  {
    const int64_t b = jvalid ? offsets[j] : 0;
    nj = jvalid ? (int32_t)(offsets[j + 1] - b) : 0;
#pragma unroll
    for (int c = 0; c < NMAX; ++c)
      boff[c] = (c < nj ? (uint32_t)codes[b + c] : 0u) * (uint32_t)(CK ? sizeof(int32_t) : sizeof(Cell));
    if (CK && ORD && NMAX <= 24) {                       // (ordered mode: four offsets per register, see nw_row_ck<.., PACKB>)
#pragma unroll
      for (int c = 0; c < NMAX; c += 4) boff[c >> 2] = boff[c] | (boff[c + 1] << 8) | (boff[c + 2] << 16) | (boff[c + 3] << 24);
    }
  }
  __syncthreads();

  const int32_t ix_first = max(NEG - goe, NEG - ge);
  const char *tab_bytes = CK ? reinterpret_cast<const char *>(tabk) : reinterpret_cast<const char *>(tab);

  // The mirrored element of row i lands in row j of the output: one lane, one row.  Storing it
  // per DP row would scatter 8-byte writes over 64 cache lines per instruction (3x write
  // amplification measured); instead a lane parks its 16 results in LDS (own slot, no sync
  // needed) and stores them as one contiguous, line-aligned run out[j][i0 .. i0+15] at the end.
  uint32_t *my_res = &mirror_res[ORD ? 0 : wave][0][lane];
  if (!ORD) {
#pragma unroll
    for (int rr = 0; rr < K3_ROWS_PER_WAVE; ++rr) my_res[rr * 64] = 0xffffffffu;  // = nothing to mirror
  }

  // (values read from LDS / derived from the wave id are wave-uniform, but the compiler cannot know: through v_readfirstlane they -- and the loop
  //  counters and addresses computed from them -- stay in SGPRs: without it the PFX kernel kept the row loop's counter, limit and residue address in
  //  VGPRs, ran the loop under an exec mask and, at five waves per SIMD, spilled the address inside the row loop)
  auto uni = [](int x) -> int { return __builtin_amdgcn_readfirstlane(x); };
  // PFX: the checkpoint (state of a row computed earlier in this wave's group at depth cp_depth) and the smallest common prefix met since
  int cp_depth = 0, since_min = 255, pfx_start = 0, pfx_save = 0;
  // the rows a wave takes: 16 consecutive ones -- or, PFX, a quarter of the tile's NEEDED rows by estimated cost, consecutive in sorted order, so that the four
  // waves of a workgroup finish together (with fixed groups of 16 -- or equal counts -- a workgroup kept its slot for its slowest wave:
  // 25 % fewer instructions gave 8 % less time)
  int it_begin = uni(wave) * K3_ROWS_PER_WAVE, it_end = it_begin + K3_ROWS_PER_WAVE;
  if (PFX) {
    // estimated DP rows of every needed row: its length minus what it shares with the previous needed row; a wave takes the consecutive
    // needed rows whose running cost falls into its quarter
    const unsigned long long need_mask = __ballot(rowneed[lane] != 0);
    int total = 0;
    {
      int mn = 255;
      bool have_prev = false;
      for (int r = 0; r < K3_TILE; ++r) {
        mn = min(mn, uni((int)rowlcp[r]));
        if ((need_mask >> r) & 1ull) {
          total += max(1, uni(rowlen[r]) - (have_prev ? mn : 0)) + 1;
          mn = 255;
          have_prev = true;
        }
      }
    }
    const int waves = K3_THREADS / 64;
    const int lo = uni(wave) * total / waves, hi = (uni(wave) + 1) * total / waves;   // this wave: rows whose running cost starts in [lo, hi)
    it_begin = it_end = 0;
    {
      int mn = 255, run = 0;
      bool have_prev = false, any = false;
      for (int r = 0; r < K3_TILE; ++r) {
        mn = min(mn, uni((int)rowlcp[r]));
        if ((need_mask >> r) & 1ull) {
          if (run >= lo && run < hi) {
            if (!any) { it_begin = r; any = true; }
            it_end = r + 1;
          }
          run += max(1, uni(rowlen[r]) - (have_prev ? mn : 0)) + 1;
          mn = 255;
          have_prev = true;
        }
      }
    }
  }
  for (int it = it_begin; it < it_end; ++it) {
    const int lr = it, rr = PFX ? 0 : it - wave * K3_ROWS_PER_WAVE;
    int64_t i = I0 + lr;
    if (i >= n) break;
    if (PFX) {
      since_min = min(since_min, uni((int)rowlcp[lr]));
      if (!uni((int)rowneed[lr])) continue;
      i = uni(rowid[lr]);
      pfx_start = (cp_depth > 0 && cp_depth <= since_min) ? cp_depth : 0;
      // the depth the NEXT needed row of this wave shares with this one: checkpoint there, if that row is computed now
      pfx_save = 0;
      {
        int mn = 255;
        for (int l2 = lr + 1; l2 < it_end; ++l2) {
          mn = min(mn, uni((int)rowlcp[l2]));
          if (uni((int)rowneed[l2])) { pfx_save = mn; break; }
        }
      }
      if (pfx_save <= pfx_start) pfx_save = 0;
    }
    if (!ordered && J0 + 63 < i) continue;  // the whole wave is below the diagonal
    if (!PFX && ordered && ti != tj && ord_first[i] >= ord_maxlast[tj]) continue;   // nothing in this row of the tile is needed
    const bool want_direct = allow_direct && i >= row_begin && i < row_end;
    const bool want_mirror_any = allow_mirror && J0 < row_end && J0 + 63 >= row_begin && (!COLS || (i >= col_begin && i < col_end));
    if (!want_direct && !want_mirror_any) continue;
    const int32_t m = uni(rowlen[lr]);

    uint32_t mt, ln;
    int32_t sc;
    if constexpr (CK) {
      constexpr int CK_S = CKBits<NMAX>::S, CK_S2 = CKBits<NMAX>::S2, CK_LB = CKBits<NMAX>::LB;
      constexpr int32_t CK_PRI = CKBits<NMAX>::PRI, CK_NEG = CKBits<NMAX>::NEG;
      // row 0 (reference :222-235) in combined form: only its max(M,Ix,Iy) feeds row 1's diagonal.
      // Iy[0][c+1] = -go - c*ge, in the moving frame (+ (c+1)*ge) the constant ge - go; no diagonal moves yet
      int32_t VM[NMAX], XP[NMAX];
      if constexpr (!ASM) {                             // (the generated block initialises its own rows; with m == 0 VM is never read)
#pragma unroll
        for (int c = 0; c < NMAX; ++c) {
          VM[c] = (ge - go) << CK_S2;
          XP[c] = 0;                                    // Ix[0][.] = -inf is handled by FIRST
        }
      }
      typedef __attribute__((address_space(3))) const uint8_t lds_u8_t;
#ifdef DA_K2_EXPERIMENTS
      if constexpr (ASM) {
        static_assert(nw_has_asm_rows<NMAX>(), "no generated row block for this NMAX");
        if (m > 0) {
          // wave-uniform operands in SGPRs; the block moves the per-cell constants into VGPRs itself (an SGPR source halves the rate of
          // v_add / v_bitop3, profiles/r04_a_ubench_inst_rate.txt)
          const uint32_t m_s = __builtin_amdgcn_readfirstlane((uint32_t)m);
          const uint32_t rc_s = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_u8_t *)&rowcodes[lr][0]);
          const uint32_t tb_s = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_u8_t *)reinterpret_cast<const uint8_t *>(tabk));
          const int32_t kx_s = ((ge - goe) << CK_S2) + (1 << CK_S), ky_s = (ge - goe) << CK_S2, pm_s = (1 << CK_S) - 1, pc_s = ~CK_PRI;
          const int32_t vi_s = (ge - go) << CK_S2, l0_s = CK_NEG << CK_S2, xf_s = ((CK_NEG - min(goe, ge)) << CK_S2) + (1 << CK_S);
          if constexpr (NMAX == 12) {
            NW_ASM_DECL_12
            asm volatile(
#include "nw_rows_p12.inc"
                : NW_ASM_OUTS_12
                : [m] "s"(m_s), [rc] "s"(rc_s), [tb] "s"(tb_s), [kx] "s"(kx_s), [ky] "s"(ky_s), [pm] "s"(pm_s), [pc] "s"(pc_s),
                  [vi] "s"(vi_s), [l0] "s"(l0_s), [xf] "s"(xf_s), NW_ASM_INS_12
                : NW_ASM_CLOBBERS_12);
            NW_ASM_COPY_12
          } else {
            NW_ASM_DECL_20
            asm volatile(
#include "nw_rows_p20.inc"
                : NW_ASM_OUTS_20
                : [m] "s"(m_s), [rc] "s"(rc_s), [tb] "s"(tb_s), [kx] "s"(kx_s), [ky] "s"(ky_s), [pm] "s"(pm_s), [pc] "s"(pc_s),
                  [vi] "s"(vi_s), [l0] "s"(l0_s), [xf] "s"(xf_s), NW_ASM_INS_20
                : NW_ASM_CLOBBERS_20);
            NW_ASM_COPY_20
          }
        }
      } else
#endif
      {
      // wave-uniform constants are parked in VGPRs: an SGPR source halves v_bitop3's issue rate
      auto in_vgpr = [](int32_t x) { int32_t v; asm volatile("v_mov_b32 %0, %1" : "=v"(v) : "s"(x)); return v; };
      const int32_t kx = in_vgpr(((ge - goe) << CK_S2) + (1 << CK_S));   // open a gap from M': -goe, +ge of the frame, priority 1
      const int32_t ky = in_vgpr((ge - goe) << CK_S2);                   // same to the left, priority 0
      const int32_t pay_mask = in_vgpr((1 << CK_S) - 1), pri_clear = in_vgpr(~CK_PRI);
      // Ix[1][c] = max(NEG-goe, NEG-ge), priority 1, payload of row 0 (nothing)
      const int32_t ixf_first = ((CK_NEG - min(goe, ge)) << CK_S2) + (1 << CK_S);
      // DIRECT sweep: sequence1's residue of the NEXT row is fetched while this row's chain runs (round 3: 466 -> 417 ms; the row loop
      // otherwise opens with ds_read_u8 + s_waitcnt lgkmcnt(0) + v_mad in front of its 20 table reads, and hipcc rotates a plain C++
      // prefetch back to that shape).  The value is in flight ACROSS two asm statements (read in one, wait in the next), so it lives in
      // a FIXED register that nothing else in the kernel names (ADVICE r3: with an ordinary "=v" variable a compiler-inserted copy or
      // spill between the two statements would capture a stale value; tests/test_nw_asm_model.py checks the disassembly: v127 appears
      // only in these statements).  LDS operations return in order, so the extra outstanding read only makes the compiler's own
      // counted lgkmcnt waits stricter.  The ordered mode does not use it (measured slower there: 98 -> 102 ms).
      constexpr bool PREFETCH = !ORD && NMAX <= 24;
      const uint32_t rc_addr = (uint32_t)(uintptr_t)(lds_u8_t *)&rowcodes[lr][0];
      register uint32_t code_v asm("v127");
      if (PREFETCH && m > 0) asm volatile("ds_read_u8 %0, %1" : "=v"(code_v) : "v"(rc_addr) : "memory");
      if (PFX && pfx_start > 0) {                                    // resume: the checkpoint's state
#pragma unroll
        for (int c = 0; c < NMAX; ++c) VM[c] = (int32_t)cp_lds[c][threadIdx.x];
#pragma unroll
        for (int c = 0; c < NMAX; c += 4) {
          const uint32_t pk = cp_lds[NMAX + c / 4][threadIdx.x];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int32_t d = (int32_t)((pk >> (8 * q)) & 0xffu);
            XP[c + q] = (int32_t)((uint32_t)((VM[c + q] >> CK_S2) - d) << CK_S2) | (1 << CK_S) | (VM[c + q] & ((1 << CK_S) - 1));
          }
        }
      }
      // the DP rows (r_from, r_to]; PFX runs them in two pieces with the checkpoint in between -- kept OUT of the row loop: with the save block inside it the
      // loop did not fit the 96 VGPRs of five waves per SIMD (three scratch reloads per DP row)
      const int32_t r_cut = (PFX && pfx_save > 0) ? pfx_save : m;      // PFX: rows (pfx_start, pfx_save], checkpoint, rows (pfx_save, m] -- ONE copy of the row loop
#pragma nounroll
      for (int piece = 0; piece < (PFX ? 2 : 1); ++piece) {
      const int32_t r_from = piece == 0 ? (PFX ? pfx_start : 0) : r_cut, r_to = piece == 0 ? r_cut : m;
      for (int32_t r = r_from + 1; r <= r_to; ++r) {
        // (making this offset opaque to the compiler turns the per-cell v_mad into a v_add but lets it
        // hoist all 20 lookups: 141 VGPRs / 3 waves per SIMD and 15 % slower -- measured, not kept)
        uint32_t row_off;
        if (PREFETCH) {
          uint32_t code_s;
          asm volatile("s_waitcnt lgkmcnt(0)\n\tv_readfirstlane_b32 %0, %1" : "=s"(code_s), "+v"(code_v) :: "memory");
          row_off = code_s * (24u * (uint32_t)sizeof(int32_t));
          asm volatile("ds_read_u8 %0, %1" : "=v"(code_v) : "v"(rc_addr + (uint32_t)(r < m ? r : r - 1)) : "memory");
        } else {
          row_off = (uint32_t)rowcodes[lr][r - 1] * (24u * (uint32_t)sizeof(int32_t));
        }
        const char *tab_row = tab_bytes + row_off;
        // column 0 of rows r-1 and r (reference :224-229): max(M,Ix,Iy)[r-1][0] = Ix = -go - (r-2)*ge (frame:
        // ge - go) and M = Iy = -inf at (r,0)
        const int32_t vm_diag0 = (r == 1) ? 0 : ((ge - go) << CK_S2);
        const int32_t left0 = CK_NEG << CK_S2;
        if (r == 1)
          nw_row_ck<NMAX, true, (ORD && NMAX <= 24)>(VM, XP, boff, tab_row, vm_diag0, left0, left0, kx, ky, ixf_first, pay_mask, pri_clear);
        else
          nw_row_ck<NMAX, false, (ORD && NMAX <= 24)>(VM, XP, boff, tab_row, vm_diag0, left0, left0, kx, ky, ixf_first, pay_mask, pri_clear);
      }
        if (PFX && piece == 0 && pfx_save > 0) {                     // the next needed row of the group shares this many rows: checkpoint
#pragma unroll
          for (int c = 0; c < NMAX; ++c) cp_lds[c][threadIdx.x] = (uint32_t)VM[c];
#pragma unroll
          for (int c = 0; c < NMAX; c += 4) {
            uint32_t pk = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) pk |= (uint32_t)min((VM[c + q] >> CK_S2) - (XP[c + q] >> CK_S2), go) << (8 * q);   // (go <= 255: the launcher's condition)
            cp_lds[NMAX + c / 4][threadIdx.x] = pk;
          }
        }
      }
      if (PFX && pfx_save > 0) { cp_depth = pfx_save; since_min = 255; }
      }
      // ---- cell (m, nj): length = m + nj - D, score = score' - (m + nj)*ge
      mt = 0; ln = (uint32_t)m;                     // nj == 0: column-0 boundary
      sc = (m == 0) ? 0 : NEG;
      if (m == 0) {
        ln = (uint32_t)nj;
        sc = (nj == 0) ? 0 : NEG;
      } else {
#pragma unroll
        for (int c = 0; c < NMAX; ++c)
          if (nj == c + 1) {
            mt = ((uint32_t)VM[c] >> CK_LB) & ((1u << (CK_S - CK_LB)) - 1u);
            ln = (uint32_t)(m + nj) - ((uint32_t)VM[c] & ((1u << CK_LB) - 1u));
            sc = (VM[c] >> CK_S2) - (m + nj) * ge;
          }
      }
    } else {
    // row 0 of the DP (reference :222-235)
    int32_t MG[NMAX], X[NMAX];
    uint32_t P[NMAX];
#pragma unroll
    for (int c = 0; c < NMAX; ++c) {
      const int32_t iy0 = -go - c * ge;  // Iy[0][c+1] = -go - ((c+1)-1)*ge
      MG[c] = max(NEG, iy0) - goe;       // max(M,Ix,Iy)[0][c+1] - goe, feeds row 1's diagonal
      X[c] = NEG;
      P[c] = (uint32_t)(c + 1);          // 0 matches, length c+1
    }
    for (int32_t r = 1; r <= m; ++r) {
      const uint32_t a = rowcodes[lr][r - 1];
      const char *tab_row = tab_bytes + a * (24u * (uint32_t)sizeof(Cell));
      // column-0 boundary of rows r-1 and r (reference :224-229)
      const int32_t hb_prev = (r == 1) ? 0 : max(NEG, -go - (r - 2) * ge);  // max(M,Ix,Iy)[r-1][0]
      const int32_t mg_diag0 = hb_prev - goe;
      const uint32_t p_diag0 = (uint32_t)(r - 1), p_left0 = (uint32_t)r;
      if (r == 1)
        nw_row<NMAX, true>(MG, X, P, boff, tab_row, mg_diag0, p_diag0, p_left0, NEG - goe, NEG, ge, goe, ix_first);
      else
        nw_row<NMAX, false>(MG, X, P, boff, tab_row, mg_diag0, p_diag0, p_left0, NEG - goe, NEG, ge, goe, ix_first);
    }

    // ---- cell (m, nj)
    uint32_t p = (uint32_t)m;  // nj == 0: length m, 0 matches (column-0 boundary)
    sc = (m == 0) ? 0 : NEG;
    if (m == 0) {              // no rows were run: the arrays still hold DP row 0
      p = (uint32_t)nj;
      sc = (nj == 0) ? 0 : NEG;
    } else {
#pragma unroll
      for (int c = 0; c < NMAX; ++c)
        if (nj == c + 1) { p = P[c]; sc = MG[c] + goe; }
    }
    mt = p >> 16;
    ln = p & 0xffffu;
    }

    if (!jvalid || (!ordered && j < i)) continue;
    const bool do_direct = want_direct && (!COLS || (j >= col_begin && j < col_end));
    const bool do_mirror = allow_mirror && (j != i) && j >= row_begin && j < row_end && (!COLS || (i >= col_begin && i < col_end));
    if (!ORD && do_mirror) my_res[rr * 64] = (mt << 16) | ln;
    if (do_direct) {
      if (f64_out) {
        reinterpret_cast<double *>(out_v)[(i + row_shift) * ld + j + col_shift] = nw_ratio(mt, ln);
      } else if (kind == DA_OUT_PACK32) {
        reinterpret_cast<uint32_t *>(out_v)[(i + row_shift) * ld + j + col_shift] = (mt << 16) | ln;
      } else {
        reinterpret_cast<uint16_t *>(out_v)[(i + row_shift) * ld + j + col_shift] = (uint16_t)((mt << 8) | (ln & 0xffu));
      }
    }
    if (score_out) {
      if (do_direct) score_out[(i + row_shift) * ld_score + j] = sc;
      if (do_mirror) score_out[(j + row_shift) * ld_score + i] = sc;
    }
  }

  // ---- mirrored run of this lane: out[j][i0 + q], q = 0..15
  if (!ORD && jvalid && allow_mirror) {
    const int64_t i0 = I0 + wave * K3_ROWS_PER_WAVE;
    const int64_t base = (j + row_shift) * ld + i0 - col_begin;
    if (f64_out) {
      double *o = reinterpret_cast<double *>(out_v) + base;
      const bool aligned = (reinterpret_cast<uintptr_t>(o) & 15) == 0;
#pragma unroll 1
      for (int q = 0; q < K3_ROWS_PER_WAVE; q += 2) {
        const uint32_t r0 = my_res[q * 64], r1 = my_res[(q + 1) * 64];
        const bool v0 = r0 != 0xffffffffu, v1 = r1 != 0xffffffffu;
        if (v0 && v1 && aligned) {
          *reinterpret_cast<double2 *>(o + q) = make_double2(nw_ratio(r0 >> 16, r0 & 0xffffu), nw_ratio(r1 >> 16, r1 & 0xffffu));
        } else {
          if (v0) o[q] = nw_ratio(r0 >> 16, r0 & 0xffffu);
          if (v1) o[q + 1] = nw_ratio(r1 >> 16, r1 & 0xffffu);
        }
      }
    } else if (kind == DA_OUT_PACK32) {
      uint32_t *o = reinterpret_cast<uint32_t *>(out_v) + base;
#pragma unroll 1
      for (int q = 0; q < K3_ROWS_PER_WAVE; ++q) {
        const uint32_t r0 = my_res[q * 64];
        if (r0 != 0xffffffffu) o[q] = r0;
      }
    } else {
      uint16_t *o = reinterpret_cast<uint16_t *>(out_v) + base;
#pragma unroll 1
      for (int q = 0; q < K3_ROWS_PER_WAVE; ++q) {
        const uint32_t r0 = my_res[q * 64];
        if (r0 != 0xffffffffu) o[q] = (uint16_t)(((r0 >> 16) << 8) | (r0 & 0xffu));
      }
    }
  }
}
