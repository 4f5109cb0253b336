// da_common.hpp -- shared host-side plumbing for libdynaalign_hip.so
// (error channel, HIP call checking, launch-geometry helpers).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../include/dynaalign.h"

namespace da {
// ---- run-time switches --------------------------------------------------------------------------------------------------------
// Every DYNAALIGN_* environment variable the library honours, parsed ONCE (first use) into this struct; INTEGRATION.md lists them.
// They select between routes / kernels that produce identical bits (tests and A / B timings use them) or size host-side resources;
// none changes a result.  da_config_reload() (a test hook, also called by the Python mirror when the process environment changed)
// parses the environment again; library code never calls getenv.
struct Config {
  // similarityMH routes (api.cpp mh_full_symmetric)
  bool mh_no_dedup = false, mh_no_sparse = false, mh_no_pipe = false, mh_pipe_one_stream = false;
  int64_t mh_dedup_min_n = -1, mh_dedup_max_pct = -1;      // -1: the built-in rule
  uint64_t mh_sparse_max_pairs = 400000000ull;
  bool mh_no_hybrid = false, mh_hybrid_dedup = false;                          // heavy / rare split of the column dictionaries (8 dense planes + incidence lists)
  int64_t mh_hybrid_min_n = -1;                            // -1: the built-in rule
  int mh_expand = 0;                                       // 0 default (first form whose shape test passes), 1 rows, 2 rowspipe, 3 pipe, 4 tiles
  int mh_pipe_step = 0, mh_pipe_wg = 0, mh_pipe_head = 0;  // 0: the built-in schedule
  int mh_expand_zones = 0;                                 // row expansion: 1 = one item list and ticket counter, else one per eighth of the output rows
  int mh_dedup_order = 0;                                  // row forms' unique ids: 0 the built-in choice, 1 first occurrence, 2 zoned (DedupOrder)
  int plane_bits = 0;                                      // lower bound on the code planes: 0 / 12 / 14 / 15 / 16, 32 = raw signature bits
  // compare kernels
  bool k2_no_asm = false, k2_persist = false;
  int k2_wg_per_cu = 0;
  // similarityNW
  bool nw_no_dedup = false, nw_int32 = false, nw_no_prefix = false;
  int64_t nw_dedup_min_n = -1;
  // host-pointer boundary
  bool no_host_widen = false, plain_d2h = false, no_buffer_cache = false;
  int d2h_threads = 0, buffer_cache_pct = 30;
  uint64_t block_bytes = 0;                                // 0: half of the free device memory
  // diagnostics / host clustering
  bool trace = false, louvain_debug = false;
  int louvain_threads = 0;
  int cc_blocks = 0;                                       // connected components: cap on the workgroups of a launch (0: 8 per CU)
};
const Config &config();


// thread-local message behind da_last_error()
std::string &last_error_ref();
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define DA_HIP_TRY(expr)                                                              \
  do {                                                                                \
    hipError_t _e = (expr);                                                           \
    if (_e != hipSuccess)                                                             \
      return ::da::fail(_e == hipErrorNoDevice || _e == hipErrorInvalidDevice         \
                            ? DA_ERR_NO_DEVICE                                        \
                            : DA_ERR_HIP,                                             \
                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),        \
                        __FILE__, __LINE__);                                          \
  } while (0)

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
// a block of `rows` rows of n keys, one workgroup per row and 32-bit chunk arithmetic: what one launch of a row-walking kernel takes
inline int block_shape_ok(int64_t rows, int64_t n) {
  if (rows > 0x7fffffffLL || n > 0x7ffffff0LL) return fail(DA_ERR_UNSUPPORTED, "key block too large for one launch");
  return DA_OK;
}

// Folded layout of one rank's shard (row-sharded multi-GPU path).  Rank p owns tile rows
// t = q*world + p (q = 0..Q-1) and only their part right of the diagonal is valid, so local
// tile rows q and Q-1-q share one stored tile row of width W = ceil8(n) + world*tile: the first
// left-aligned from its diagonal tile, the second starting at column shard_back(W, n) = W - ceil8(n)
// (so both start on a multiple of 8 columns: 16-byte loads of row pieces stay aligned).  That
// halves the bytes the all-gather has to move.
struct ShardGeom {
  int64_t n, W, rows;  // rows = local rows per rank
  int world, tile, T, Q, Qh;
};
__host__ __device__ inline int64_t shard_back(int64_t W, int64_t n) { return W - ((n + 7) / 8) * 8; }   // local column of global column 0 in a back-aligned row
inline ShardGeom shard_geom(int64_t n, int world, int tile) {
  ShardGeom g;
  g.n = n; g.world = world; g.tile = tile;
  g.T = (int)ceil_div(n, tile);
  g.Q = (int)ceil_div(g.T, world);
  g.Qh = (g.Q + 1) / 2;
  g.W = ceil_div(n, 8) * 8 + (int64_t)world * tile;
  g.rows = (int64_t)g.Qh * tile;
  return g;
}

// ---- layout of the bit-plane operand of k_mh_compare (written by dict_kernels.hip) -------------
// The compare kernel stages, per 128-row tile and per stage (SP planes = SEGS 16-byte units per row),
// 128 x SEGS units into LDS with wave-wide DMA instructions of 64 consecutive units.  The operand
// is therefore stored in exactly that order -- [block of 128 rows][stage][LDS slot][unit] -- so a
// DMA instruction reads 1 KiB of consecutive memory (8 full lines) instead of 16..21 separate row
// pieces.  Slot order and the XOR swizzle of 64-byte slots are the kernel's LDS image:
//   slot of tile row r: ((r>>5)*2 + (r&1))*16 + ((r&31)>>1)   (the 16 lanes of a ds_read_b128
//   group hit consecutive slots);  unit position of logical segment s: s ^ ((slot>>2)&3) if SEGS == 4.
// Two copies: rows (planes in order) and, `copy_words` further, columns (each plane pair swapped).
__host__ __device__ inline int k2_slot(int r) { return (((r >> 5) * 2 + (r & 1)) << 4) + ((r & 31) >> 1); }
__host__ __device__ inline int k2_row_of_slot(int s) { return ((s >> 5) << 5) + ((s & 15) << 1) + ((s >> 4) & 1); }
struct PlaneGeom {
  int pl;       // planes per group of 32 hash functions: 8, 12, 16 (dictionary codes) or 32 (raw)
  int sp;       // planes per stage (pl, or 16 when pl = 32)
  int segs;     // 16-byte units per row per stage
  int nst;      // stages: groups x stages per group
  int64_t blocks, copy_words;
};
__host__ __device__ inline PlaneGeom plane_geom(int64_t n, int n_hash, int pl) {
  PlaneGeom g;
  g.pl = pl; g.sp = pl == 32 ? 16 : pl; g.segs = g.sp / 4;
  g.nst = ((n_hash + 31) / 32) * (pl / g.sp);
  g.blocks = (n + 127) / 128;
  g.copy_words = g.blocks * g.nst * 128 * g.sp;
  return g;
}
// word offset (inside one copy) of the 16-byte unit holding logical segment `seg` of `row` in stage `st`
__host__ __device__ inline int64_t plane_unit_word(const PlaneGeom &g, int64_t row, int st, int seg) {
  const int rs = k2_slot((int)(row & 127));
  const int xs = g.segs == 4 ? (rs >> 2) & 3 : 0;
  return ((((row >> 7) * g.nst + st) * 128 + rs) * g.segs + (seg ^ xs)) * 4;
}
// The hand-scheduled 16-plane kernel (k_mh_compare_a16) reads a PADDED twin of the 16-plane operand, stored behind the two
// regular copies: same [block of 128 rows][stage][LDS slot] order, but 80-byte slots (16 plane words + 4 words of padding):
// its 8-byte operand reads are then bank-conflict-free at plain immediate offsets and a wave's share of a stage is five 1 KiB
// DMA pieces.  Row copy: plane p at word p; column copy: word p ^ 1 (pair-swapped like the regular column copy).
constexpr int K2_PAD16_SLOT_WORDS = 20;
__host__ __device__ inline int64_t pad16_copy_words(int64_t n, int n_hash) {
  return ((n + 127) / 128) * (int64_t)((n_hash + 31) / 32) * 128 * K2_PAD16_SLOT_WORDS;
}
__host__ __device__ inline int64_t pad16_base_words(int64_t n, int n_hash) { return 2 * plane_geom(n, n_hash, 16).copy_words; }
__host__ __device__ inline int64_t pad16_slot_word(int64_t n, int n_hash, int64_t row, int group) {   // first word of the row's slot
  const int64_t nst = (n_hash + 31) / 32;
  return (((row >> 7) * nst + group) * 128 + k2_slot((int)(row & 127))) * K2_PAD16_SLOT_WORDS;
}
// uint32 words an operand buffer must hold for any plane count (raw 32 planes, or 16 planes + their padded twin)
inline int64_t mh_planes_words(int64_t n, int n_hash) {
  if (n <= 0 || n_hash <= 0) return 0;
  const int64_t raw = 2 * plane_geom(n, n_hash, 32).copy_words;
  const int64_t p16 = pad16_base_words(n, n_hash) + 2 * pad16_copy_words(n, n_hash);
  return raw > p16 ? raw : p16;
}

// ---- the packed U x U count table of the row expansion (n_hash <= 511: every count fits 9 bits) -------------------------------
// Row r holds pk_lo_bytes(U) low bytes (column c at byte c), then one byte of bit 8 per 8 columns (column c at bit c & 7 of byte c >> 3):
// exactly k_expand_stream's LDS image of the row.  The low plane is a whole number of 128-column tiles, so a compare tile owns one 128-byte
// piece of the low plane and one 16-byte piece of the bit plane of each of its rows; the row stride stays a multiple of 16 bytes.
__host__ __device__ inline int64_t pk_lo_bytes(int64_t U) { return (U + 127) / 128 * 128; }
__host__ __device__ inline int64_t pk_row_bytes(int64_t lo_bytes) { return lo_bytes + lo_bytes / 8; }
inline size_t pk_table_bytes(int64_t U) { return (size_t)U * (size_t)pk_row_bytes(pk_lo_bytes(U)); }

// ---- zones of the row expansion (minhash_kernels.hip "ROW expansion") and the duplicate plan's zoned id order --------------------
// The output rows are cut into `zones` contiguous ranges of zone_rows() rows each (ES_ZONES, one per XCD; 1 = no zoning).  The copy lists
// (es_layout) and the plan's zoned numbering (k_dd_assign) both take the zone height from here, so they cannot disagree.
constexpr int ES_ZONES = 8;
__host__ __device__ inline int64_t zone_rows(int64_t n, int zones) { return (n + zones - 1) / zones; }
// Zoned order of the single-copy strings: zone z holds h[z] of them, and the q-th one of zone z (in row order) gets the rank of (q, z) among
// all pairs {(q', z') : q' < h[z']} in lexicographic order -- the singles dealt round-robin over the zones, an exhausted zone skipped.
// Exact integers: sum over z' of min(q, h[z']) pairs have a smaller q', and one pair per zone z' < z with h[z'] > q shares q.
__host__ __device__ inline int64_t zoned_rank(const int32_t *h, int zones, int z, int64_t q) {
  int64_t r = 0;
  for (int t = 0; t < zones; ++t) r += ((int64_t)h[t] < q ? (int64_t)h[t] : q) + ((t < z && (int64_t)h[t] > q) ? 1 : 0);
  return r;
}

// Kernel launchers implemented in the .hip translation units.  All are
// asynchronous on `stream`; argument checking is done by the C-ABI layer.
int launch_minhash_signatures(const uint8_t *d_res, const int64_t *d_off, int64_t n,
                              int k, int n_hash, const uint32_t *d_seeds, uint32_t *d_sig,
                              int64_t ld_sig, hipStream_t stream);
int launch_mh_compare(const uint32_t *d_planes, int64_t n, int n_hash,
                      int64_t row_begin, int64_t row_end, bool symmetric, int kind,
                      void *d_out, int64_t ld, hipStream_t stream, int plane_bits = 32, int tile_stride = 1,
                      bool upper_only = false, int fold_q = 0, int64_t fold_w = 0);
// rows [row_begin, row_end) x columns [col_begin, col_end) of the pair space, each element stored once (da_dev_mh_compare_rect)
int launch_mh_compare_rect(const uint32_t *d_planes, int64_t n, int n_hash, int64_t row_begin, int64_t row_end, int64_t col_begin, int64_t col_end,
                           int kind, void *d_out, int64_t ld, hipStream_t stream, int plane_bits);
// rows [m, m_pad) of a signature matrix <- copies of its first rows (the two-set operand [x ; pad ; y])
int launch_fill_sig_rows(uint32_t *d_sig, int64_t ld_sig, int64_t m, int64_t m_pad, int n_hash, hipStream_t stream);
// the symmetric uint16 12-plane compare in pieces (pipelined duplicate route): tile-row bands of 8 x 128 rows, taken in order
int64_t mh_sym_bands(int64_t n);
int64_t mh_sym_band_prefix(int64_t n, int64_t band);
bool mh_compare_bands_ok(int64_t n, int n_hash, int plane_bits, const void *d_out, int64_t ld);
// (pk: d_out is the packed table (pk_*), ld its pk_lo_bytes; 12 planes only)
int launch_mh_compare_bands_u16(const uint32_t *d_planes, int64_t n, int n_hash, uint16_t *d_out, int64_t ld, int64_t band_begin,
                                int64_t band_end, int wg_per_cu, hipStream_t stream, int plane_bits = 12, bool pk = false);
int launch_mh_compare_edges_u16(const uint32_t *d_planes, int64_t n, int n_hash, uint16_t *d_out, int64_t ld, hipStream_t stream, int plane_bits = 12,
                                bool pk = false);
// the whole symmetric 12-plane compare into the packed table, one tile per workgroup (the one-stream row form)
bool mh_compare_pk_ok(int64_t n, int n_hash, int plane_bits);
int launch_mh_compare_pk(const uint32_t *d_planes, int64_t n, int n_hash, uint8_t *d_tab, hipStream_t stream);
// minhash_kernels.hip, SPARSE route of the symmetric float64 compare (inputs whose signatures rarely agree): see the kernels' header comment
size_t mh_sparse_pairs_limit();
int launch_mh_sparse_count(const uint16_t *d_idsT, int64_t ld_ids, int64_t n, int n_hash, int max_ids, unsigned long long *d_stats, hipStream_t stream);
size_t mh_sparse_scratch_words(int64_t n, int n_hash, int max_ids, int64_t ld_ids);
int launch_mh_sparse(const uint16_t *d_idsT, int64_t ld_ids, int64_t n, int n_hash, int max_ids, uint64_t pairs, uint32_t *d_scratch,
                     uint32_t *d_entries32, uint16_t *d_entries, double *d_out, int64_t ld, hipStream_t stream, hipEvent_t after_buckets = nullptr);
// ... its list phase alone (k_sp_classes .. k_sp_band: the matching incidences of the codes in d_idsT, bucketed per 128 x 128 tile on or above the
// diagonal), and the kernel that ADDS those incidences to a finished dense result (heavy / rare split: the dense compare saw the heavy values only)
int launch_mh_sparse_lists(const uint16_t *d_idsT, int64_t ld_ids, int64_t n, int n_hash, int max_ids, uint64_t pairs, uint32_t *d_scratch,
                           uint32_t *d_entries32, uint16_t *d_entries, hipStream_t stream);
int launch_mh_sparse_fixup(const uint32_t *d_scratch, const uint16_t *d_entries, int64_t n, int n_hash, int max_ids, int64_t ld_ids, int kind, void *d_out,
                           int64_t ld, int64_t tile_row_begin, int64_t tile_row_end, hipStream_t stream);
// dict_kernels.hip: where the codes of launch_mh_dictionary sit in its workspace ([n_hash][*ld_ids] uint16, 0xFFFF = value seen once)
const uint16_t *mh_dictionary_codes(const void *d_work, int64_t n, int n_hash, int64_t *ld_ids);
// dict_kernels.hip: signatures -> compare operand.  Dictionary codes (8 / 12 / 16 planes per group,
// whatever the largest column dictionary needs) are exact for n <= DA_DICT_MAX_N; *d_status_out
// points at two ints in the workspace ({error, largest id count}), valid once the stream has drained.
constexpr int64_t DA_DICT_MAX_N = 131068;
size_t mh_planes_workspace_bytes(int64_t n, int n_hash);
int launch_mh_dictionary(const uint32_t *d_sig, int64_t ld_sig, int64_t n, int n_hash, void *d_work,
                         int **d_status_out, hipStream_t stream);
int mh_plane_bits_for(int max_ids);
int launch_ids_to_planes(const void *d_work, int64_t n, int n_hash, int plane_bits, uint32_t *d_planes,
                         hipStream_t stream, const uint16_t *d_codes = nullptr);
// heavy / rare split of the column dictionaries (dict_kernels.hip k_hy_split): dense codes for 8 planes + sparse codes for the incidence lists
int launch_mh_heavy_split(void *d_work, int64_t n, int n_hash, int max_ids, int keep, const uint16_t **d_dense_out, const uint16_t **d_sparse_out,
                          unsigned long long *d_stats, hipStream_t stream);
int launch_sig_to_planes(const uint32_t *d_sig, int64_t ld_sig, int64_t n, int n_hash, uint32_t *d_planes,
                         hipStream_t stream);
int launch_finalize_sharded(const uint16_t *d_g, int64_t ld_g, const ShardGeom &geom, bool is_nw, int n_hash,
                            double *d_out, int64_t ld, hipStream_t stream);   // interior tiles: k_finalize_rows (16-byte stores)
int64_t shard_packed_bytes(const ShardGeom &g, int value_bits);
int launch_shards_to_table(const void *d_g, int64_t ld_g, const ShardGeom &geom, int value_bits, uint16_t *d_table, int64_t ld,
                           hipStream_t stream);
int launch_pack_shard(const uint16_t *d_local, int64_t ld, const ShardGeom &geom, int value_bits, uint8_t *d_packed,
                      hipStream_t stream);
int launch_finalize_packed(const uint8_t *d_g, const ShardGeom &geom, int value_bits, int n_hash, double *d_out, int64_t ld,
                           hipStream_t stream);
int launch_nw_encode(const uint8_t *d_res, int64_t total, uint8_t *d_codes, int32_t *d_bad,
                     hipStream_t stream);
int launch_nw(const uint8_t *d_codes, const int64_t *d_off, int64_t n, int64_t max_len,
              int matrix_id, int gap_open, int gap_ext, int64_t row_begin, int64_t row_end,
              bool symmetric, int kind, void *d_out, int64_t ld, int32_t *d_score,
              int64_t ld_score, hipStream_t stream, int shard_rank = 0, int shard_world = 0,
              const int32_t *ord_first = nullptr, const int32_t *ord_minfirst = nullptr, const int32_t *ord_maxlast = nullptr,
              const int32_t *ord_perm = nullptr, const uint8_t *ord_lcp = nullptr,   // ord_perm / ord_lcp: launch_nw_sort_unique (prefix sharing)
              int64_t col_begin = 0, int64_t col_end = -1);                          // row-block mode: only the columns [col_begin, col_end) (-1: n)
// the row-block mode by name: rows [r0, r1) x columns [c0, c1) of the pair space, no scores, no shard, no ordering
inline int launch_nw_rect(const uint8_t *d_codes, const int64_t *d_off, int64_t n, int64_t max_len, int matrix_id, int gap_open, int gap_ext,
                          int64_t r0, int64_t r1, int64_t c0, int64_t c1, int kind, void *d_out, int64_t ld, hipStream_t stream) {
  return launch_nw(d_codes, d_off, n, max_len, matrix_id, gap_open, gap_ext, r0, r1, false, kind, d_out, ld, nullptr, 0, stream, 0, 0, nullptr, nullptr,
                   nullptr, nullptr, nullptr, c0, c1);
}
// nw_kernels.hip: lexicographic order of (unique) sequences of <= 24 residues + the common prefix of sorted neighbours, for the ordered DP
size_t nw_sort_unique_workspace_bytes(int64_t n);
int launch_nw_sort_unique(const uint8_t *d_codes, const int64_t *d_off, int64_t n, void *d_work, size_t work_bytes, const int32_t **perm_out,
                          const uint8_t **lcp_out, hipStream_t stream);
// nw_kernels.hip: collapse byte-identical sequences before the N x N sweep (exact; see the kernels' header comment)
// The start slot of a string in the plan's open-addressing table is dd_hash & (table_size - 1); host-callable so that the tests' model
// (tests/unique_plan_model.py, through da_debug_dd_hash) can build probe chains on purpose.
__host__ __device__ __forceinline__ uint32_t dd_hash(const uint8_t *c, int64_t b, int32_t len) {
  uint32_t h = 0x9747b28cu ^ (uint32_t)len;
  for (int32_t q = 0; q < len; ++q) { h ^= c[b + q]; h *= 0x01000193u; h ^= h >> 15; }
  h ^= h >> 13; h *= 0x5bd1e995u; h ^= h >> 15;
  return h;
}
struct NwDedupPlan {
  uint32_t *table; uint32_t table_size;
  int32_t *rep, *mult, *last, *fm, *fs, *pm, *ps, *uid_of, *uidx, *ufirst, *ulast, *ulen, *minfirst, *maxlast;
  int64_t *uoff;
  uint8_t *ucodes;
  size_t bytes;
};
NwDedupPlan nw_dedup_layout(void *work, int64_t n, int64_t total);
size_t nw_dedup_workspace_bytes(int64_t n, int64_t total);
int launch_nw_dedup_count(const uint8_t *d_codes, const int64_t *d_off, int64_t n, const NwDedupPlan &p, hipStream_t stream);
// How the unique strings are numbered (every order is a permutation of [0, U); equal strings share an id):
//   multi_first  multi-copy strings (ids < M) in order of first occurrence, then the single-copy ones in order of occurrence: NW's plan
//   first        every string by first occurrence: rows [0, R) of the input only use ids < pm[R] + ps[R] (MinHash's tile forms)
//   zoned        multi-copy strings as above, then the single-copy ones dealt round-robin over the `zones` row zones of zone_rows(n, zones)
//                rows (zoned_rank): every band of the table holds about as many singles of each zone (MinHash's row forms)
enum class DedupOrder { multi_first = 0, first = 1, zoned = 2 };
int launch_nw_dedup_build(const uint8_t *d_codes, const int64_t *d_off, int64_t n, int64_t U, const NwDedupPlan &p, hipStream_t stream,
                          DedupOrder order = DedupOrder::multi_first, int zones = 1);   // zones (1 ... ES_ZONES): the zoned order's
// minhash_kernels.hip: out[i][j] = value(D[uidx[min(i,j)]][uidx[max(i,j)]]) for the dense symmetric n x n result
int launch_expand_unique(const uint16_t *d_D, int64_t ld_d, const int32_t *d_uidx, int64_t n, int kind, bool is_nw, int n_hash,
                         void *d_out, int64_t ld, hipStream_t stream, int nw_max_len = 0, uint16_t *d_F = nullptr,
                         const int32_t *d_ufirst = nullptr, int64_t U = 0, hipEvent_t after_gather = nullptr, hipEvent_t after_rows = nullptr,
                         int table_world = 1, int64_t table_rows_local = 0,    // table_world > 1: d_D is all-gathered row blocks of cyclic 128-row units
                         bool only_leftover = false);                          // true: the caller ran launch_gather_columns / launch_expand_rows itself
// ROW expansion (MinHash: symmetric table): every output row written once from its table row held in LDS; no gathered copy
bool expand_stream_ok(int64_t n, int64_t U, int n_hash, const void *d_out, int64_t ld);
size_t expand_stream_scratch_bytes(int64_t n, int64_t U);
bool expand_stream_packed(int n_hash);   // the LDS row is packed to 9 bits per count: two K2 rings fit beside it
int expand_stream_zones();               // the zones of a call's copy lists: ES_ZONES, or 1 (DYNAALIGN_MH_EXPAND_ZONES=1)
// (pk: d_D is the packed table (pk_*) and ld_d its pk_lo_bytes; needs expand_stream_packed)
int launch_expand_stream(const uint16_t *d_D, int64_t ld_d, const int32_t *d_uidx, int64_t n, int64_t U, int n_hash, double *d_out, int64_t ld,
                         void *d_scratch, hipStream_t stream, hipEvent_t after_lists = nullptr, bool pk = false);
int launch_expand_stream_lists(const int32_t *d_uidx, int64_t n, int64_t U, void *d_scratch, hipStream_t stream);
// the rectangular form (two sets collapsed per side): out[i][j] = D[ux(i)][uy(j)] / n_hash, D the U_x x U_y uint16 table (ld_d >= U_y, a multiple of
// 8); d_scratch: expand_stream_scratch_bytes(m, U_x)
bool expand_stream_rect_ok(int64_t m, int64_t n, int64_t U_x, int64_t U_y, int n_hash, const void *d_out, int64_t ld);
int launch_expand_stream_rect(const uint16_t *d_D, int64_t ld_d, const int32_t *d_uidx_x, int64_t m, int64_t U_x, const int32_t *d_uidx_y, int64_t n,
                              int64_t U_y, int n_hash, double *d_out, int64_t ld, void *d_scratch, hipStream_t stream,
                              hipEvent_t after_lists = nullptr);
int launch_expand_stream_rows(const uint16_t *d_D, int64_t ld_d, const int32_t *d_uidx, int64_t n, int64_t U, int n_hash, double *d_out, int64_t ld,
                              void *d_scratch, int64_t row_end, hipStream_t stream,   // the items below table row row_end that earlier launches left
                              bool pk = false);
int launch_expand_rows(const uint16_t *d_F, int64_t ld_f, const int32_t *d_uidx, int64_t n, bool is_nw, int n_hash, int nw_max_len,
                       double *d_out, int64_t ld, int64_t band_begin, int64_t band_end, hipStream_t stream);
// bytes of the column-gathered table (d_F) that switches launch_expand_unique to its two streaming passes; 0 = shape not covered
size_t expand_rows_workspace_bytes(int64_t n, int64_t U, int kind, bool is_nw, int n_hash, int nw_max_len);
int launch_upper_histogram(const uint16_t *d_m, int64_t ld, int64_t n, int nbins, unsigned long long *d_hist,
                           hipStream_t stream, int rank = 0, int world = 0, const int32_t *d_rowmap = nullptr);
int launch_extract_edges(const uint16_t *d_m, int64_t ld, int64_t n, const uint8_t *d_keep, int nbins,
                         bool include_diagonal, int32_t *d_i, int32_t *d_j, uint16_t *d_v, int64_t capacity,
                         unsigned long long *d_count, hipStream_t stream, int rank = 0, int world = 0,
                         const int32_t *d_rowmap = nullptr);
// minhash_kernels.hip: F[r][j] = D[r][uidx[j]] for the columns right of (from_first_tile: from) the 128-tile of r's first occurrence
int launch_gather_columns(const uint16_t *d_D, int64_t ld_d, const int32_t *d_uidx, const int32_t *d_ufirst, int64_t n, int64_t U,
                          uint16_t *d_F, int64_t ld_f, bool from_first_tile, hipStream_t stream, int table_world = 1,
                          int64_t table_rows_local = 0, int64_t row_begin = 0, int64_t row_end = -1);
// graph_kernels.hip: (i <= j, code) edge list -> symmetric CSR sorted by (row, column); diagonal entries -> loops[] (0xFFFF = none)
size_t edges_to_csr_workspace_bytes(int64_t m, int64_t n);
int launch_edges_to_csr(const int32_t *d_i, const int32_t *d_j, const uint16_t *d_v, int64_t m, int64_t n, void *d_work, size_t work_bytes,
                        int64_t *d_ptr, int32_t *d_adj, uint16_t *d_codes, uint16_t *d_loops, hipStream_t stream);
// louvain_kernels.hip: the synchronous Louvain of clusterbreak.louvain_sync_dense on a canonical CSR in device memory (da_dev_louvain_csr)
size_t louvain_device_workspace_bytes(int64_t n, int64_t nnz);
int launch_louvain_device(int64_t n, const int64_t *d_ptr, const int32_t *d_adj, const uint16_t *d_codes, const uint16_t *d_loops, const double *values,
                          int n_values, double resolution, uint32_t seed, void *d_work, size_t work_bytes, int32_t *d_membership, double *modularity_out,
                          int32_t *levels_out, int32_t *iterations_out, hipStream_t stream);
// components_kernels.hip: connected components (clusterbreak.components_dense) by a lock-free union-find whose roots are the component minima
// (components_common.hpp), then ids from 1 in order of first appearance (da_dev_components_*).  launch_cc_init / launch_cc_finish frame a
// union launch of the caller's (launch_lsh_union): parent[v] = v into the workspace; compression, renumbering, optional sizes (n entries)
// and the number of components.  The finish and the two whole calls synchronise the stream.  1 <= n <= 2^31 - 16.
size_t components_workspace_bytes(int64_t n);
int components_max_blocks();   // workgroups of a grid-stride launch of this family
int launch_cc_init(int64_t n, void *d_work, size_t work_bytes, int32_t **d_parent_out, hipStream_t stream);
int launch_cc_finish(int64_t n, void *d_work, size_t work_bytes, int32_t *d_membership, int32_t *d_sizes, int64_t *n_components_out,
                     hipStream_t stream);
int launch_components_edges(const int32_t *d_i, const int32_t *d_j, const uint16_t *d_code, int min_code, int64_t m, int64_t n, void *d_work,
                            size_t work_bytes, int32_t *d_membership, int32_t *d_sizes, int64_t *n_components_out, hipStream_t stream);
int launch_components_csr(int64_t n, const int64_t *d_ptr, const int32_t *d_adj, bool symmetric, void *d_work, size_t work_bytes,
                          int32_t *d_membership, int32_t *d_sizes, int64_t *n_components_out, hipStream_t stream);
// graph_kernels.hip: nearest-neighbour lists (n rows of ld >= top columns and their uint16 keys) -> the (i <= j, code) edge list of their union /
// mutual kNN graph, the diagonal first in every row's share when `loops` (da_dev_knn_edges); d_i / d_j / d_v hold n * (top + loops) entries
size_t knn_edges_workspace_bytes(int64_t n, int top);
int launch_knn_edges(const int32_t *d_idx, const uint16_t *d_key, int64_t ld, int64_t n, int top, bool mutual, bool is_nw, const uint16_t *d_self_key,
                     int self_code, bool loops, void *d_work, size_t work_bytes, int32_t *d_i, int32_t *d_j, uint16_t *d_v, uint64_t *d_count,
                     hipStream_t stream);
// topk_kernels.hip: per-row exact top-k of uint16 keys by (rank descending, column ascending) (da_dev_topk_rows); index and key rows have
// their own leading dimensions.  ... and the selected MinHash counts as doubles: d_val[r * ld_val + t] = d_key[r * ld_key + t] / n_hash
constexpr int DA_TOPK_MAX = 1024;
int launch_topk_rows(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, const uint16_t *d_rank, int rank_bits, int top, int32_t *d_idx,
                     int64_t ld_idx, uint16_t *d_key_out, int64_t ld_key, hipStream_t stream);
// ... with every row's own column left out of the selection: the block's row r owns column self_col0 + r (a row block of a square problem), and
// its key goes to d_self_key[r] when that pointer is given; 1 <= top <= n - 1 (da_dev_topk_rows_self)
int launch_topk_rows_self(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, const uint16_t *d_rank, int rank_bits, int top, int64_t self_col0,
                          int32_t *d_idx, int64_t ld_idx, uint16_t *d_key_out, int64_t ld_key, uint16_t *d_self_key, hipStream_t stream);
// ... and the same selection on uint32 keys that are value ranks below nbins (da_dev_topk_ranks[_self]): nbins only places the 8-bit digits
int launch_topk_ranks(const uint32_t *d_keys, int64_t rows, int64_t n, int64_t ld, int64_t nbins, int top, int32_t *d_idx, int64_t ld_idx,
                      uint32_t *d_key_out, int64_t ld_key, hipStream_t stream);
int launch_topk_ranks_self(const uint32_t *d_keys, int64_t rows, int64_t n, int64_t ld, int64_t nbins, int top, int64_t self_col0, int32_t *d_idx,
                           int64_t ld_idx, uint32_t *d_key_out, int64_t ld_key, uint32_t *d_self_key, hipStream_t stream);
int launch_topk_values(const uint16_t *d_key, int64_t ld_key, int64_t rows, int top, int n_hash, double *d_val, int64_t ld_val, hipStream_t stream);
// rect_edges_kernels.hip: the threshold form of a two-set rectangle, on a block of `rows` rows of ld >= n uint16 keys (da_dev_rect_histogram,
// da_dev_threshold_rows_count / _emit): histogram of the whole block; per-row count of the keys flagged in d_keep + exclusive scan -> row
// pointers; the flagged columns of every row in ascending order at its row pointer.  ... and the kept MinHash counts as doubles
size_t threshold_rows_workspace_bytes(int64_t rows);
int launch_rect_histogram(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, int nbins, unsigned long long *d_hist, hipStream_t stream);
int launch_threshold_rows_count(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, const uint8_t *d_keep, int nbins, int64_t *d_rowptr,
                                void *d_work, size_t work_bytes, hipStream_t stream);
int launch_threshold_rows_emit(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, const uint8_t *d_keep, int nbins, const int64_t *d_rowptr,
                               int32_t *d_j, uint16_t *d_key_out, int64_t capacity, hipStream_t stream);
// the same steps on blocks of uint32 keys -- PACK32 codes (matches << 16 | length) to value ranks through the table of da_nw_value_ranks and
// the rank histogram (nw_edges_long_kernels.hip), and the ordered compaction of the keys >= r_min (rect_edges_kernels.hip).  triangle: the
// block is rows [row_begin, ...) x columns [col_begin, ...) of a square problem; the histogram counts global column > global row, count /
// emit keep global column >= global row.
int launch_nw_codes_to_ranks(const uint32_t *d_codes, int64_t rows, int64_t n, int64_t ld, int max_len, const uint32_t *d_rank, uint32_t *d_out,
                             int64_t ld_out, hipStream_t stream);
int launch_rank_histogram(const uint32_t *d_keys, int64_t rows, int64_t n, int64_t ld, int64_t nbins, unsigned long long *d_hist, bool triangle,
                          int64_t row_begin, int64_t col_begin, hipStream_t stream);
int launch_threshold_ranks_count(const uint32_t *d_keys, int64_t rows, int64_t n, int64_t ld, uint32_t r_min, int64_t nbins, bool triangle,
                                 int64_t row_begin, int64_t col_begin, int64_t *d_rowptr, void *d_work, size_t work_bytes, hipStream_t stream);
int launch_threshold_ranks_emit(const uint32_t *d_keys, int64_t rows, int64_t n, int64_t ld, uint32_t r_min, int64_t nbins, bool triangle,
                                int64_t row_begin, int64_t col_begin, const int64_t *d_rowptr, int32_t *d_j, uint32_t *d_key_out, int64_t capacity,
                                hipStream_t stream);
// stats_kernels.hip: per row of a block of keys (the origin convention of launch_rank_histogram), over the elements with global column > global
// row, the smallest and the largest rank with the first local column holding each, and the rank of the diagonal element (da_dev_upper_extrema[32])
int launch_upper_extrema(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, const uint16_t *d_rank, int64_t row_begin, int64_t col_begin,
                         da_row_extrema *d_rec, hipStream_t stream);
int launch_upper_extrema32(const uint32_t *d_keys, int64_t rows, int64_t n, int64_t ld, int64_t row_begin, int64_t col_begin, da_row_extrema *d_rec,
                           hipStream_t stream);
int launch_edge_values(const uint16_t *d_key, int64_t count, int n_hash, double *d_w, hipStream_t stream);
// d_out[r] = d_in[r] + base for r < count (a block's row pointers placed into the row pointers of the whole rectangle)
int launch_rowptr_offset(const int64_t *d_in, int64_t count, int64_t base, int64_t *d_out, hipStream_t stream);
// nw_align_kernels.hip: the alignment path of listed pairs (da_dev_nw_align_pairs), one lane per pair; entries [pair_base, pair_base + pairs) of the
// lists (NULL lists: pair p is x[p] against y[p]); output pointers are those of entry pair_base.  Launches as many pairs as the workspace holds at a time.
size_t nw_align_workspace_bytes(int64_t pairs);
int launch_nw_align(const uint8_t *d_x_codes, const int64_t *d_x_off, int64_t m, const uint8_t *d_y_codes, const int64_t *d_y_off, int64_t n,
                    const int32_t *d_pair_x, const int32_t *d_pair_y, int64_t pair_base, int64_t pairs, int matrix_id, int gap_open, int gap_ext,
                    uint8_t *d_ops, int64_t ld_ops, int32_t *d_len, int32_t *d_matches, int32_t *d_score, void *d_work, size_t work_bytes,
                    hipStream_t stream);
// nw_align_long_kernels.hip: the same for sequences of up to 1024 residues (da_dev_nw_align_long_pairs), one wavefront per pair in one persistent
// launch; a slot of nw_align_long_slot_bytes(max_len) bytes per wave in flight, none without d_ops.
size_t nw_align_long_slot_bytes(int64_t max_len);
size_t nw_align_long_workspace_bytes(int64_t pairs, int64_t max_len);
int launch_nw_align_long(const uint8_t *d_x_codes, const int64_t *d_x_off, int64_t m, const uint8_t *d_y_codes, const int64_t *d_y_off, int64_t n,
                         const int32_t *d_pair_x, const int32_t *d_pair_y, int64_t pair_base, int64_t pairs, int matrix_id, int gap_open, int gap_ext,
                         uint8_t *d_ops, int64_t ld_ops, int32_t *d_len, int32_t *d_matches, int32_t *d_score, int64_t max_len, void *d_work,
                         size_t work_bytes, hipStream_t stream);
// nw_lsh_kernels.hip: NW (matches, length) of a resident pair list over two encoded sets, split on the device into the lane-per-pair and the
// wavefront-per-pair kernels above (da_dev_nw_rescore_pairs); a refused pair -- an index outside its set, a length of 0 or over 1024 --
// gets -1 / -1.  The workspace is nw_rescore_fixed_bytes(pairs) (lists, classes, scan; 256 spare bytes for any alignment) plus the
// lane-per-pair kernel's decision words for the short pairs in flight: at least one wavefront of them (minimal), a smaller share means more
// launches and never another result.  counts_host = {short, long, refused}.  Synchronises the stream once (the class totals are read back);
// the alignment launches and the scatter behind it are asynchronous.
size_t nw_rescore_fixed_bytes(int64_t pairs);
size_t nw_rescore_workspace_bytes(int64_t pairs, bool minimal);
int launch_nw_rescore(const uint8_t *d_x_codes, const int64_t *d_x_off, int64_t m, const uint8_t *d_y_codes, const int64_t *d_y_off, int64_t n,
                      const int32_t *d_i, const int32_t *d_j, int64_t pairs, int matrix_id, int gap_open, int gap_ext, int32_t *d_matches,
                      int32_t *d_length, void *d_work, size_t work_bytes, int64_t counts_host[3], hipStream_t stream);
// ... and the threshold list of it (da_dev_lsh_nw_edges): the sorted 64-bit keys of the LSH back end unpacked, keep[p] = matches >=
// min_matches[length] with the kept counts per chunk of 64 and their exclusive sum (chunks + 1 entries each; d_temp: nwl_keep_scan_bytes),
// and the kept (i, j, matches, length) written in listed order, the first `capacity` of them
int launch_nwl_split(const uint64_t *d_key, int64_t count, int32_t *d_i, int32_t *d_j, hipStream_t stream);
size_t nwl_keep_scan_bytes(int64_t pairs);
int launch_nwl_keep(const int32_t *d_matches, const int32_t *d_length, int64_t pairs, const int32_t *d_min_matches, int table_len, uint8_t *d_keep,
                    int64_t *d_chunk_kept, int64_t *d_chunk_off, void *d_temp, size_t temp_bytes, hipStream_t stream);
int launch_nwl_emit(const int32_t *d_i, const int32_t *d_j, const int32_t *d_matches, const int32_t *d_length, const uint8_t *d_keep,
                    const int64_t *d_chunk_off, int64_t pairs, int64_t capacity, int32_t *d_out_i, int32_t *d_out_j, int32_t *d_out_matches,
                    int32_t *d_out_length, hipStream_t stream);
// ... and the nearest-neighbour lists of it (da_dev_lsh_nw_knn): the value rank of every pair's (matches, length), the keep byte (rank >=
// r_min and rank > 0), the diagonal of one set taken aside; d_totals[2] = {kept pairs, pairs without a rank}
int launch_nwl_rank_keys(const int32_t *d_i, const int32_t *d_j, const int32_t *d_matches, const int32_t *d_length, int64_t pairs, const uint32_t *d_rank,
                         int max_len, uint32_t r_min, bool one_set, int64_t n_diag, uint32_t *d_key, uint8_t *d_keep, uint32_t *d_diag_key,
                         uint64_t *d_totals, hipStream_t stream);
// consensus_kernels.hip: the center-star consensus of a pooled cluster table (da_dev_cluster_consensus and its pieces).  Pairs are numbered per
// cluster i ascending then j != i ascending (d_pair_ptr: the running sums of c (c - 1), int64), rows (center, j != center) j ascending.
// launch_cons_pairs lists entries [p0, p1) of the pairs (d_center == NULL) or of the rows; launch_cons_center_sums ADDS the fixed-point terms of
// pairs [p0, p1) to the two 64-bit limbs of their members (the host copies of the two tables find the members the block touches);
// launch_cons_pick rounds the limbs to 53 bits and writes every cluster's center as a pooled index; launch_cons_vote tallies the ops rows
// [q_lo, q_hi) for clusters [k0, k0 + kcount) and writes the consensus letters of every cluster whose rows end inside the range.
int launch_cons_pair_ptr(const int64_t *d_cluster_ptr, int64_t clusters, int64_t *d_pair_ptr, hipStream_t stream);
int launch_cons_pairs(const int64_t *d_cluster_ptr, const int64_t *d_pair_ptr, int64_t clusters, const int32_t *d_center, int64_t p0, int64_t p1,
                      int32_t *d_pair_x, int32_t *d_pair_y, hipStream_t stream);
int launch_cons_center_sums(const int32_t *d_len, const int32_t *d_matches, int64_t p0, int64_t p1, const int64_t *cluster_ptr_host,
                            const int64_t *pair_ptr_host, const int64_t *d_cluster_ptr, const int64_t *d_pair_ptr, int64_t clusters, uint64_t *d_sums,
                            hipStream_t stream);
int launch_cons_pick(const uint64_t *d_sums, const int64_t *d_cluster_ptr, int64_t clusters, int32_t *d_center, hipStream_t stream);
int launch_cons_vote(const uint8_t *d_codes, const int64_t *d_off, const int64_t *d_cluster_ptr, const int32_t *d_center, int64_t k0, int64_t kcount,
                     const uint8_t *d_ops, int64_t ld_ops, const int32_t *d_len, int64_t q_lo, int64_t q_hi, uint32_t *d_carry, uint8_t *d_cons,
                     int64_t ld_cons, int32_t *d_cons_len, int64_t max_len, hipStream_t stream);
size_t cluster_consensus_workspace_bytes(const int64_t *cluster_ptr_host, int64_t clusters, int64_t max_len, bool minimal);
int launch_cluster_consensus(const uint8_t *d_codes, const int64_t *d_off, int64_t n, const int64_t *cluster_ptr_host, const int64_t *d_cluster_ptr,
                             int64_t clusters, int64_t max_len, int matrix_id, int gap_open, int gap_ext, uint8_t *d_cons, int64_t ld_cons,
                             int32_t *d_cons_len, int32_t *d_center, void *d_work, size_t work_bytes, hipStream_t stream);
// jaccard_kernels.hip: the exact Jaccard index of k-shingle sets (da_dev_jaccard_sets / da_dev_jaccard_rect).  Keys are uint32 for k <= 4 and uint64
// for k 5 .. 8; a set is the ascending distinct keys of a sequence, [n][ld_keys] keys + [n] uint8 counts, ld_keys >= jaccard_sets_ld(max_len, k).
// The rectangle is rows x columns of ONE set operand, DA_OUT_COMPACT (intersection << 8 | union) or DA_OUT_F64.
int64_t jaccard_sets_ld(int64_t max_len, int k);
int launch_jaccard_sets(const uint8_t *d_res, const int64_t *d_off, int64_t n, int64_t max_len, int k, void *d_keys, int64_t ld_keys, uint8_t *d_counts,
                        hipStream_t stream);
int launch_jaccard_rect(const void *d_keys, const uint8_t *d_counts, int64_t n, int64_t ld_keys, int k, int64_t row_begin, int64_t row_end, int64_t col_begin,
                        int64_t col_end, int kind, void *d_out, int64_t ld, hipStream_t stream);
// jaccard_long_kernels.hip: the same for sequences of up to 1024 shingle positions (da_dev_jaccard_sets_long / da_dev_jaccard_rect_long): uint16
// counts, ld_keys up to 1024, and the rectangle as DA_OUT_PACK32 (intersection << 16 | union) or DA_OUT_F64.
int64_t jaccard_sets_long_ld(int64_t max_len, int k);
int launch_jaccard_sets_long(const uint8_t *d_res, const int64_t *d_off, int64_t n, int64_t max_len, int k, void *d_keys, int64_t ld_keys,
                             uint16_t *d_counts, hipStream_t stream);
int launch_jaccard_rect_long(const void *d_keys, const uint16_t *d_counts, int64_t n, int64_t ld_keys, int k, int64_t row_begin, int64_t row_end,
                             int64_t col_begin, int64_t col_end, int kind, void *d_out, int64_t ld, hipStream_t stream);
// lev_kernels.hip: the Levenshtein similarity in its bit-parallel form (da_dev_lev_masks / da_dev_lev_rect), sequences of at most 127 bytes.
// class_map (host, 256 entries) maps a byte to its class id below n_classes; the operand is one buffer of lev_masks_bytes(n, max_len, n_classes)
// bytes holding match masks, texts and lengths.  The rectangle is rows x columns of ONE operand, DA_OUT_COMPACT ((L - d) << 8 | L) or DA_OUT_F64.
size_t lev_masks_bytes(int64_t n, int64_t max_len, int n_classes);
int launch_lev_masks(const uint8_t *d_res, const int64_t *d_off, int64_t n, int64_t max_len, const uint8_t *class_map, int n_classes, void *d_masks,
                     size_t masks_bytes, hipStream_t stream);
int launch_lev_rect(const void *d_masks, int64_t n, int64_t max_len, int n_classes, int64_t row_begin, int64_t row_end, int64_t col_begin, int64_t col_end,
                    int kind, void *d_out, int64_t ld, hipStream_t stream);
// MinHash LSH banding (da_dev_lsh_*).  Elements are (sequence, band) pairs, rows * bands <= LSH_MAX_ELEMENTS of them; an INCIDENCE is a pair
// of sequences that share a bucket in one band.  A front end numbers the incidences as the slots of an exclusive sum, describes them in
// an LshSlots and reads back their number and its statistics; the caller checks the cap and sizes the per-incidence buffers; the back end
// (lsh_kernels.hip) verifies the slots -- row i of sig_a against row j of sig_b -- and turns the kept ones into a sorted edge list or into
// ragged rows for the nearest-neighbour selection.  The two front ends:
//   one set   lsh_buckets (lsh_kernels.hip): keys, a sort and the partner counts inside the workspace; sig_a = sig_b, every slot has i < j,
//             and the edge list carries the n diagonal entries;
//   two sets  lsh_cross_probe (lsh_cross_kernels.hip): the INDEX of a resident set y is its sorted (band key, id) elements with a table of
//             where every band starts (layout: include/dynaalign.h); nothing in it depends on the queries.  A query batch x PROBES it:
//             element q = i * bands + t finds the run of its key, lo[q] / len[q], and the exclusive sum of len numbers the incidences.
constexpr int64_t LSH_MAX_ELEMENTS = 0x7fffff00LL;
// slot s belongs to the element e with off[e] <= s < off[e + 1]; which (i, j, band) that is depends on the front end:
//   !probed  e is a position of the sorted elements: i = ids[e], j = ids[e + 1 + s - off[e]], band = keys[e] >> 48
//   probed   e = i * bands + band, j = ids[lo[e] + s - off[e]]
struct LshSlots {
  bool probed;
  const int64_t *off;     // [elements + 1]: the exclusive sum of the partner counts / the probed lengths
  const int32_t *ids;     // the sorted ids: of the workspace's sort / of the index
  const uint64_t *keys;   // !probed: the sorted keys
  const uint32_t *lo;     // probed: [elements], where the run of element e starts in ids
  int64_t elements;       // rows * bands
  int bands;
};
size_t lsh_workspace_bytes(int64_t n, int bands);
int launch_lsh_band_keys(const uint32_t *d_sig, int64_t n, int64_t ld_sig, int bands, int rows, uint64_t *d_keys, int32_t *d_ids, hipStream_t stream);
// keys, sort, partner counts and their exclusive sum inside the workspace; reads back stats_host = {largest bucket, buckets} and the incidences
int lsh_buckets(const uint32_t *d_sig, int64_t n, int64_t ld_sig, int bands, int rows, void *d_work, size_t work_bytes, LshSlots *slots_out,
                uint32_t stats_host[2], int64_t *incidences_host, hipStream_t stream);
int launch_lsh_verify_listed(const uint32_t *d_sig_a, int64_t rows_a, int64_t ld_a, const uint32_t *d_sig_b, int64_t rows_b, int64_t ld_b, int n_hash,
                             int bands, int rows, uint32_t c_min, const int32_t *d_i, const int32_t *d_j, const int32_t *d_band, int64_t triples,
                             uint16_t *d_count, uint8_t *d_keep, hipStream_t stream);
size_t lsh_chunk_scan_bytes(int64_t incidences);
int launch_lsh_verify_enumerated(const uint32_t *d_sig_a, int64_t rows_a, int64_t ld_a, const uint32_t *d_sig_b, int64_t rows_b, int64_t ld_b, int n_hash,
                                 int rows, uint32_t c_min, const LshSlots &slots, int64_t incidences, uint16_t *d_count, uint8_t *d_keep,
                                 int64_t *d_chunk_kept, int64_t *d_chunk_off, uint64_t *d_distinct, void *d_temp, size_t temp_bytes, hipStream_t stream);
size_t lsh_edge_sort_bytes(int64_t edges);
// edges = diagonal_n + the last entry of the chunk offsets; diagonal_n = the rows of one set, 0 for two sets
int launch_lsh_emit_sort(const LshSlots &slots, int64_t rows_a, int64_t diagonal_n, int n_hash, int64_t incidences, const uint16_t *d_count,
                         const uint8_t *d_keep, const int64_t *d_chunk_off, int64_t edges, uint64_t *d_key_in, uint16_t *d_val_in, uint64_t *d_key_out,
                         uint16_t *d_val_out, void *d_temp, size_t temp_bytes, hipStream_t stream);
int launch_lsh_split(const uint64_t *d_key, const uint16_t *d_val, int64_t count, int32_t *d_i, int32_t *d_j, uint16_t *d_count, hipStream_t stream);
// ... and the components of the same graph (da_dev_lsh_components): the union step over the kept slots, into the parent array of launch_cc_init
int launch_lsh_union(const LshSlots &slots, int64_t incidences, const uint8_t *d_keep, int32_t *d_parent, hipStream_t stream);
// ... and the nearest-neighbour lists from the same candidates (da_dev_lsh_knn*, da_dev_lsh_cross_topk): after the verify step,
// launch_lsh_knn_entries turns the kept slots into ragged rows (both: the two directions of every pair of one set, entries = 2 * kept;
// otherwise the rows of x, entries = kept) and launch_lsh_knn_select takes every row's first `top` entries by (count descending, column
// ascending) -- rows of up to 64 entries by a wave, longer ones by a workgroup, which sorts up to 2048 entries whole and radix-selects in
// longer rows.  The selection needs no workspace and does not synchronise.
size_t lsh_knn_scan_bytes(int64_t n);
int launch_lsh_knn_entries(const LshSlots &slots, int64_t rows_a, bool both, int64_t incidences, const uint16_t *d_count, const uint8_t *d_keep,
                           int64_t entries, int top, int64_t *d_cursor, int64_t *d_ptr, int32_t *d_col, uint16_t *d_cnt, uint64_t *d_written, void *d_temp,
                           size_t temp_bytes, hipStream_t stream);
int launch_lsh_knn_select(const int64_t *d_ptr, int64_t nnz, const int32_t *d_col, const uint16_t *d_count, int64_t n, int top, int32_t *d_idx,
                          int64_t ld_idx, uint16_t *d_key, int64_t ld_key, hipStream_t stream);
int launch_lsh_knn_written(const int64_t *d_ptr, int64_t n, int64_t nnz, int top, uint64_t *d_written, hipStream_t stream);
// the same two steps with a uint32 payload, the NW value ranks (da_dev_lsh_nw_knn, da_dev_nw_knn_select): the entries come from an unpacked
// candidate list (d_i, d_j, rank key and keep byte per pair), the selection orders (rank descending, column ascending)
int launch_nw_knn_entries(const int32_t *d_i, const int32_t *d_j, int64_t pairs, const uint32_t *d_rank_key, const uint8_t *d_keep, int64_t rows_a,
                          bool both, int64_t entries, int top, int64_t *d_cursor, int64_t *d_ptr, int32_t *d_col, uint32_t *d_val, uint64_t *d_written,
                          void *d_temp, size_t temp_bytes, hipStream_t stream);
int launch_nw_knn_select(const int64_t *d_ptr, int64_t nnz, const int32_t *d_col, const uint32_t *d_rank_key, int64_t n, int top, int32_t *d_idx,
                         int64_t ld_idx, uint32_t *d_key, int64_t ld_key, hipStream_t stream);
// lsh_cross_kernels.hip: the index and the probe (da_dev_lsh_index_*, and the front end of da_dev_lsh_cross_*)
struct LshIndexView {
  const uint32_t *meta, *band_start;
  const uint64_t *keys;
  const int32_t *ids;
};
size_t lsh_index_bytes(int64_t n, int bands);
LshIndexView lsh_index_view(const void *d_index, int64_t n, int bands);
size_t lsh_index_build_scratch_bytes(int64_t n, int bands);
int lsh_index_build(const uint32_t *d_sig, int64_t n, int64_t ld_sig, int bands, int rows, void *d_index, void *d_scratch, hipStream_t stream);
size_t lsh_cross_workspace_bytes(int64_t m, int bands);
// probe into caller arrays (d_lo / d_len int32 [m * bands]; d_stats: 16 bytes of scratch); *mismatch_host = 1 when the index was built for
// another (n, bands, rows).  Synchronises.
int lsh_index_probe_listed(const void *d_index, int64_t n, const uint32_t *d_sig_x, int64_t m, int64_t ld_x, int bands, int rows, int32_t *d_lo,
                           int32_t *d_len, uint32_t *d_stats, int *mismatch_host, hipStream_t stream);
// probe + exclusive sum inside the workspace; reads back stats_host = {largest probed run, runs of the index, mismatch} and the incidences
int lsh_cross_probe(const void *d_index, int64_t n, const uint32_t *d_sig_x, int64_t m, int64_t ld_x, int bands, int rows, void *d_work, size_t work_bytes,
                    LshSlots *slots_out, uint32_t stats_host[3], int64_t *incidences_host, hipStream_t stream);
int launch_symmetrize(void *d_mat, int64_t n, int64_t ld, int kind, hipStream_t stream);
int launch_acc_counts(uint32_t *d_acc, const uint16_t *d_cnt, int64_t count, bool first, hipStream_t stream);
int launch_counts32_to_f64(const uint32_t *d_acc, double *d_out, int64_t count, int n_hash, hipStream_t stream);
int launch_widen(const uint16_t *d_in, double *d_out, int64_t count, bool is_nw, int n_hash,
                 hipStream_t stream);

}  // namespace da
