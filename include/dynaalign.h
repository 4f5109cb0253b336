/*
 * dynaalign.h -- C ABI of libdynaalign_hip.so (MI355X / gfx950 HIP kernels).
 *
 * This is the drop-in boundary for DynaAlign's all-pairs similarity hot path.
 * The reference crosses from R into native code through two Rcpp-generated
 * .Call entry points (reference src/RcppExports.cpp:15-25 and :28-39) that
 * convert SEXPs and call
 *     NumericMatrix similarityMH(CharacterVector, int k, int n_hash)
 *                                        reference src/minHash.cpp:119-188
 *     NumericMatrix similarityNW(CharacterVector, std::string, int, int)
 *                                        reference src/pairwiseSeqAlign.cpp:331-365
 * The functions below replace the BODIES of those two functions.  The R-level
 * signatures (reference R/RcppExports.R:15-17, :34-36) and the .Call symbols
 * stay exactly as they are; the Rcpp glue that binds them to this ABI is in
 * r_glue/ and described in INTEGRATION.md.
 *
 * Conventions
 *   - plain C types only; no exceptions, no library-owned memory crosses.
 *   - sequences are passed packed: `residues` holds the raw bytes of all
 *     sequences back to back, `offsets[i]..offsets[i+1]` delimits sequence i
 *     (n+1 entries).  This is what the glue builds once from the STRSXP
 *     (the reference instead copies per element: src/minHash.cpp:147,
 *     src/pairwiseSeqAlign.cpp:341-343).
 *   - every function returns DA_OK (0) or a DA_ERR_* code; da_last_error()
 *     returns the message for the calling thread.  For the reference's own
 *     error conditions the message text is the reference's, verbatim.
 *   - N x N results are symmetric, so row- and column-major coincide: `out`
 *     may be R's REAL() pointer (reference allocates NumericMatrix(n,n) at
 *     src/minHash.cpp:134 / src/pairwiseSeqAlign.cpp:335).
 *   - "host" functions take host pointers and do their own H2D/D2H; "dev"
 *     functions take DEVICE pointers (hipMalloc'ed by the caller, e.g. a
 *     torch tensor's data_ptr()) plus a hipStream_t passed as void*, launch
 *     asynchronously on that stream and never synchronise.
 *   - there is NO CPU fallback: without a usable HIP device every compute
 *     entry point fails with DA_ERR_NO_DEVICE.
 */
#ifndef DYNAALIGN_H
#define DYNAALIGN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* (round 4 added entry points only -- da_config_reload, da_debug_comm_cache_state, da_mh_last_route_split: the version stays)
 * (the two-set entry points -- da_similarity_*_cross, da_dev_*_rect, da_dev_similarity_mh_cross, da_mh_cross_last_route -- were added likewise)
 * (the two-set top-k entry points -- da_similarity_*_cross_topk, da_dev_similarity_mh_cross_topk, da_dev_topk_rows, da_nw_code_ranks -- likewise)
 * (the one-set nearest-neighbour entry points -- da_similarity_*_knn, da_dev_similarity_mh_knn, da_dev_topk_rows_self, da_dev_knn_edges[_bytes] -- likewise)
 * (the two-set threshold entry points -- da_similarity_*_cross_edges_begin, da_dev_similarity_mh_cross_edges, da_dev_rect_histogram,
 *  da_dev_threshold_rows_* -- likewise)
 * (the alignment-path entry points -- da_nw_align_pairs, da_dev_nw_align_pairs, da_nw_align_workspace_bytes and their _long forms -- likewise)
 * (the cluster-consensus entry points -- da_cluster_consensus, da_dev_cluster_consensus[_workspace_bytes], da_dev_consensus_[center_sums | pick |
 *  vote] -- likewise)
 * (the exact-Jaccard entry points -- da_similarity_jaccard[_cross[_topk] | _knn | _edges[_begin]], da_dev_jaccard_sets[_ld], da_dev_jaccard_rect -- likewise)
 * (their _long forms -- da_similarity_jaccard[_cross[_topk | _edges] | _knn | _edges | _stats]_long[_begin], da_jaccard_sets_long_ld,
 *  da_dev_jaccard_sets_long, da_dev_jaccard_rect_long -- likewise)
 * (the LSH entry points -- da_similarity_mh_lsh_edges_begin, da_similarity_mh_lsh_knn, da_mh_lsh_last_route,
 *  da_dev_lsh_[band_keys | verify_pairs | edges | knn | knn_select | workspace_bytes] -- likewise)
 * (the two-set LSH entry points -- da_similarity_mh_lsh_cross_[edges_begin | topk], da_dev_lsh_index_[bytes | build | probe],
 *  da_dev_lsh_cross_[verify_pairs | workspace_bytes | edges | topk] -- likewise)
 * (the connected-components entry points -- da_components, da_dev_components_[workspace_bytes | edges | csr], da_dev_lsh_components,
 *  da_similarity_mh_lsh_components -- likewise)
 * (the NW-on-LSH-candidates entry points -- da_similarity_nw_lsh_[cross_]edges_begin, da_dev_lsh_[cross_]nw_edges,
 *  da_dev_nw_rescore_pairs, da_dev_nw_rescore_workspace_bytes, da_nw_lsh_last_route -- likewise)
 * (the NW-ranked LSH list entry points -- da_similarity_nw_lsh_knn, da_similarity_nw_lsh_cross_topk, da_dev_lsh_nw_knn,
 *  da_dev_lsh_cross_nw_topk, da_dev_nw_knn_select, da_dev_nw_rank_keys -- likewise)
 * (the Levenshtein entry points -- da_similarity_lev[_cross[_topk | _edges_begin] | _knn | _edges[_begin]], da_dev_lev_masks[_bytes],
 *  da_dev_lev_rect -- likewise)
 * 2: the folded shard layout changed (da_shard_ld = ceil8(n) + world * 128, back-aligned rows start at column world * 128) and the
 *    duplicate-route / multi-device entry points were added; every round-1 entry point keeps its signature */
#define DA_ABI_VERSION 2

enum da_status {
  DA_OK = 0,
  DA_ERR_EMPTY_INPUT = 1,      /* "Input sequences vector cannot be empty"     src/minHash.cpp:121-123 */
  DA_ERR_BAD_K = 2,            /* "'k' must be a positive integer"             src/minHash.cpp:125-127 */
  DA_ERR_BAD_NHASH = 3,        /* "Number of hash functions must be positive"  src/minHash.cpp:129-131 */
  DA_ERR_BAD_MATRIX = 4,       /* "Invalid substitution matrix name: %s"       src/pairwiseSeqAlign.cpp:204 */
  DA_ERR_BAD_RESIDUE_SEQ1 = 5, /* "Invalid amino acid in sequence1: %c"        src/pairwiseSeqAlign.cpp:241-243 */
  DA_ERR_BAD_RESIDUE_SEQ2 = 6, /* "Invalid amino acid in sequence2: %c"        src/pairwiseSeqAlign.cpp:248-250 */
  DA_ERR_NOMEM = 7,
  DA_ERR_NO_DEVICE = 8,        /* no HIP device / runtime: the product has no CPU path */
  DA_ERR_HIP = 9,              /* a HIP call failed; message carries hipGetErrorString */
  DA_ERR_UNSUPPORTED = 10,     /* outside what the gfx950 kernels implement (message says what) */
  DA_ERR_BAD_ARG = 11
};

/* element type of a device-side similarity block */
enum da_out_kind {
  DA_OUT_F64 = 0,    /* double: MH matches/n_hash (src/minHash.cpp:174), NW matches/len (src/pairwiseSeqAlign.cpp:311) */
  DA_OUT_COMPACT = 1, /* uint16: MH match count; NW (matches << 8 | len) -- valid for len <= 255 */
  DA_OUT_PACK32 = 2   /* uint32, NW only: (matches << 16 | len) -- any supported length */
};

const char *da_last_error(void);
const char *da_status_message(int status); /* static text for a code ("" if none) */
int da_abi_version(void);
int da_device_count(void); /* 0 when no HIP device is usable */
/* The library parks its large device buffers (>= 1 MiB; per device at most 16 buffers totalling at most 30 % of the device's
 * memory (DYNAALIGN_BUFFER_CACHE_PCT changes the share) -- the 80 GB result buffer costs seconds to allocate, and one call of the duplicate-collapsing routes uses four
 * large buffers) for the next call instead of returning them to the driver.  Parked memory is invisible to other allocators
 * in the process (e.g. PyTorch's): this call hands everything back.  An allocation of the library's own that would
 * otherwise fail releases the parked buffers first.  Returns the bytes freed. */
size_t da_release_device_memory(void);
/* Run-time switches.  The library reads its DYNAALIGN_* environment variables (INTEGRATION.md lists them: route / kernel selection
 * between forms that produce identical bits, sizes of host-side resources, tracing) ONCE, at its first use, into one struct.
 * da_config_reload parses the environment again -- a hook for tests and A / B timing scripts that flip a switch inside one process
 * (the Python mirror calls it by itself when the process's DYNAALIGN_* environment changed since its last call). */
void da_config_reload(void);
/* Test hook for the communicator cache of DA_EXCHANGE_ALLGATHER (the communicators of a device list are kept between calls; a call in which
 * some rank failed destroys its list's entry, since a communicator that saw an abandoned collective may hang the next one):
 * out2 = {cached device lists, entries destroyed after a failed call}; force_fail != 0 makes rank 0 of the next ALLGATHER call fail
 * before the collective. */
int da_debug_comm_cache_state(int force_fail, size_t *out2);

/* ---- HashFamily (reference src/minHash.cpp:67-89) ------------------------ */

/* seeds_out[h] = h-th raw output of std::mt19937(seed)  (src/minHash.cpp:75-80). */
int da_hash_family_seeds(uint32_t seed, int n_hash, uint32_t *seeds_out);
/* what the reference's default argument does: std::random_device{}() (src/minHash.cpp:73). */
uint32_t da_random_seed(void);

/* ---- host-pointer entry points (what the Rcpp glue calls) ---------------- */

/* similarityMH body (src/minHash.cpp:119-188).  `seeds` = n_hash hash seeds
 * (da_hash_family_seeds); validation order and messages as :121-131.
 * out: n*n doubles, diagonal exactly 1.0 (:161). */
int da_similarity_mh(const uint8_t *residues, const int64_t *offsets, int64_t n,
                     int k, int n_hash, const uint32_t *seeds, double *out);

/* ---- the same two bodies on several GPUs of the node, ONE process (SURVEY 8(b) "da_opts", 8(e)) ----
 * opts == NULL behaves like da_similarity_mh / da_similarity_nw on the current device.  With a device list, a host
 * thread per device runs the pipeline on its GPU and copies ITS rows of the result into `out` (P PCIe links instead
 * of one).  `exchange` selects how the pair space is split and reassembled:
 *   DA_EXCHANGE_ROWS       device p computes the contiguous row block it copies out; no device-to-device traffic
 *                          (default; the same device may be listed more than once);
 *   DA_EXCHANGE_ALLGATHER  cyclic upper-triangle shards (da_dev_*_shard), ONE ncclAllGather over xGMI (RCCL,
 *                          ncclCommInitAll on the list), mirror + widen to the full matrix on every device;
 *   DA_EXCHANGE_PEERCOPY   the same shards, exchanged by concurrent hipMemcpyPeerAsync reads of every peer's block
 *                          (xGMI is point-to-point: all links at once; no RCCL needed).
 * NW with an exchange needs sequences of <= 64 residues (uint16 shard codes); ROWS has the limits of da_similarity_nw.
 * phase_ms (optional, DA_PHASE_COUNT doubles): per phase the maximum over devices, in ms --
 *   [0] upload + signatures/codes (+ ncclCommInitAll on the first call with a device list: the communicators are cached until
 *   da_release_device_memory())  [1] compare / NW  [2] exchange  [3] finalize  [4] device-to-host  [5] whole call, from entry.
 * The R glue builds this struct from options(DynaAlign.devices = , DynaAlign.exchange = ) (r_glue/). */
enum da_exchange { DA_EXCHANGE_ROWS = 0, DA_EXCHANGE_ALLGATHER = 1, DA_EXCHANGE_PEERCOPY = 2 };
#define DA_PHASE_COUNT 6
typedef struct da_opts {
  uint32_t struct_size;      /* sizeof(da_opts) -- lets the struct grow without breaking callers */
  int32_t n_devices;         /* 0: the current device */
  const int32_t *devices;    /* HIP device ordinals */
  int32_t exchange;          /* enum da_exchange */
  uint32_t reserved;         /* 0 */
  double *phase_ms;          /* NULL or DA_PHASE_COUNT doubles (out) */
} da_opts;
int da_similarity_mh_opts(const uint8_t *residues, const int64_t *offsets, int64_t n,
                          int k, int n_hash, const uint32_t *seeds, double *out, const da_opts *opts);
int da_similarity_nw_opts(const uint8_t *residues, const int64_t *offsets, int64_t n,
                          const char *matrix_name, int gap_open, int gap_ext, double *out, const da_opts *opts);
/* 1 when librccl can be bound in this process (DA_EXCHANGE_ALLGATHER usable), else 0. */
int da_rccl_available(void);

/* The signature matrix alone (src/minHash.cpp:140-157): sig_out[n][n_hash]. */
int da_minhash_signatures(const uint8_t *residues, const int64_t *offsets, int64_t n,
                          int k, int n_hash, const uint32_t *seeds, uint32_t *sig_out);

/* Integer match counts (the numerator at src/minHash.cpp:168-174) for rows
 * [row_begin,row_end) x all n columns; counts_out[rows][n]; diagonal = n_hash.
 * Requires n_hash <= 65535. */
int da_mh_counts(const uint8_t *residues, const int64_t *offsets, int64_t n,
                 int k, int n_hash, const uint32_t *seeds,
                 int64_t row_begin, int64_t row_end, uint16_t *counts_out);

/* similarityNW body (src/pairwiseSeqAlign.cpp:331-365): BLOSUM name lookup
 * (:190-206), pair (i,j), i<=j, evaluated as calc(seq[i], seq[j]) (:340-346),
 * mirrored (:349-350), diagonal computed.  n == 0 returns DA_OK and writes
 * nothing (the reference returns a 0x0 matrix).  Residue errors reproduce the
 * reference's first-raised message (lazy row-major validation, :238-250). */
int da_similarity_nw(const uint8_t *residues, const int64_t *offsets, int64_t n,
                     const char *matrix_name, int gap_open, int gap_ext, double *out);

/* The integers behind similarityNW for rows [row_begin,row_end) x all n
 * columns, each entry for calc(seq[min(i,j)], seq[max(i,j)]):
 *   matches_out / len_out : the two operands of the divide at :311
 *   score_out             : M[m][n] after the fill (:268-278), never exposed
 *                           by the reference -- auxiliary, may be NULL.
 * Arrays are [rows][n] int32; any may be NULL. */
int da_nw_pairs(const uint8_t *residues, const int64_t *offsets, int64_t n,
                const char *matrix_name, int gap_open, int gap_ext,
                int64_t row_begin, int64_t row_end,
                int32_t *matches_out, int32_t *len_out, int32_t *score_out);

/* ---- two sets: x (m sequences) against y (n sequences), an m x n float64 matrix R ---------
 * What a caller does after clustering one set: compare a second set against it (new peptides against a library, one probe array
 * against another, consensus sequences against members).
 *   MinHash: R[i][j] = (double)#{h : sig_x[i][h] == sig_y[j][h]} / (double)n_hash, signatures, seeds and k-mers exactly those of
 *            similarityMH (src/minHash.cpp:140-157, :174): bit for bit the block [0:m, m:m+n] of similarityMH(c(x, y), k, n_hash) under
 *            the same seeds.  NO forced diagonal: R[i][j] is 1.0 only because the signatures agree.
 *   NW:      R[i][j] = calc(x[i], y[j]) with x[i] as sequence1 (src/pairwiseSeqAlign.cpp:209-313): bit for bit the block [0:m, m:m+n] of
 *            similarityNW(c(x, y), ...).  NaN where both strings are empty, 0.0 where exactly one is.
 * column_major = 0 writes out[i * n + j]; 1 writes out[i + j * m] (R's NumericMatrix(m, n)); neither involves a host-side transpose.
 * Validation, before any device is needed -- MinHash: x empty, then y empty (DA_ERR_EMPTY_INPUT), then k, then n_hash.  NW: the matrix
 * name first; m == 0 or n == 0 returns DA_OK and writes nothing; residue errors are what the reference's lazy fill would raise first
 * with the pairs visited i ascending over x and j ascending over y, each pair in calc's own order (:238-250: seq1[0], every character of
 * seq2, seq1[1], ...; an empty x[i] checks nothing, an empty y[j] still has every character of x[i] checked).
 * Limits: n_hash <= 65535 (DA_ERR_UNSUPPORTED beyond: the host-side chunking of da_similarity_mh is not carried over); NW sequence lengths
 * as da_similarity_nw; more than 131 068 rows in the joint operand (m rounded up to a multiple of 128, + n) take the raw 32-plane
 * operand, like n > 131 068 in da_dev_mh_planes -- still exact.  When only the padding of x pushes the joint operand over that bound
 * (m + n <= 131 068 < m rounded up + n), x is left unpadded: the dictionary codes are kept and the compiled compare kernel serves the call
 * (the column origin is then not a multiple of 128).  Single device; without one, DA_ERR_NO_DEVICE after validation.
 * The host calls work in row blocks of DYNAALIGN_BLOCK_BYTES sized by the column count alone (a tall result is not cut by its width); for
 * MinHash the device block has an even leading dimension, so odd column counts keep the hand-scheduled kernels. */
int da_similarity_mh_cross(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m,
                           const uint8_t *y_residues, const int64_t *y_offsets, int64_t n,
                           int k, int n_hash, const uint32_t *seeds, double *out, int column_major);
int da_similarity_nw_cross(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m,
                           const uint8_t *y_residues, const int64_t *y_offsets, int64_t n,
                           const char *matrix_name, int gap_open, int gap_ext, double *out, int column_major);

/* ---- two sets, top-k per row: the `top` most similar y for every x, without the m x n matrix ----
 * R is the matrix da_similarity_mh_cross / da_similarity_nw_cross return.  Row i of the result lists `top` columns j of row i of R, ordered
 * by R[i][j] descending and, among equal values, by j ascending: numpy's argsort(-R, axis = 1, kind = "stable")[:, :top].  Columns of
 * similarity 0 are ordinary entries (they fill a row with fewer than `top` positive columns); no forced diagonal.
 *   idx_out : [m][top] int32, 0-based columns;  val_out : [m][top] float64 or NULL, val[i][t] bit for bit R[i][idx[i][t]]
 *             (MinHash (double)count / (double)n_hash, NW (double)matches / (double)length).
 * Equal VALUES tie even when their integer codes differ (NW 2/4 and 3/6): the device selects on the dense rank of a code's double value
 * (da_nw_code_ranks; the identity on MinHash counts), never on the raw code.
 * Validation, before any device is needed: everything da_similarity_*_cross checks, in its order and with its texts; then top < 1 or
 * top > n -> DA_ERR_BAD_ARG, top > 1024 -> DA_ERR_UNSUPPORTED (da_dev_topk_rows).  NW: m == 0 returns DA_OK; n == 0 with m > 0 is
 * DA_ERR_BAD_ARG (no top satisfies 1 <= top <= 0); like da_similarity_nw_edges every sequence on both sides has 1 .. 127 residues
 * (DA_ERR_UNSUPPORTED: the uint16 code holds an 8-bit alignment length, and an empty sequence's similarities are NaN / 0.0 -- a NaN has
 * no place in an order).  Only m x top numbers leave the device: the rectangle is computed as uint16 codes in row blocks of
 * DYNAALIGN_BLOCK_BYTES (sized by the column count alone) and selected from there.  Single device, the direct route only. */
int da_similarity_mh_cross_topk(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m,
                                const uint8_t *y_residues, const int64_t *y_offsets, int64_t n,
                                int k, int n_hash, const uint32_t *seeds, int top, int32_t *idx_out, double *val_out);
int da_similarity_nw_cross_topk(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m,
                                const uint8_t *y_residues, const int64_t *y_offsets, int64_t n,
                                const char *matrix_name, int gap_open, int gap_ext, int top, int32_t *idx_out, double *val_out);

/* The value-rank table of the NW codes (matches << 8 | length) of sequences up to max_len (1 .. 127) residues: rank_out[code], 65536
 * entries, is the dense rank (0 = smallest) of (double)matches / (double)length among the codes with 1 <= length <= 2 * max_len and
 * matches <= min(length, max_len) -- equal doubles get equal ranks, a larger double a larger rank.  Codes outside that set cannot occur
 * and get rank 0.  *distinct_out (may be NULL): the number of ranks.  Host only; needs no device. */
int da_nw_code_ranks(int max_len, uint16_t *rank_out, int *distinct_out);

/* ---- one set, nearest-neighbour lists: for every sequence its `top` most similar OTHER sequences, without the n x n matrix ----
 * S is the matrix da_similarity_mh / da_similarity_nw return (n x n, symmetric).  Row i of the result lists the `top` columns j != i ordered
 * by S[i][j] descending and, among equal values, by j ascending: numpy's argsort(-S', axis = 1, kind = "stable")[:, :top] with S' = S whose
 * diagonal is -inf.  Columns of similarity 0 are ordinary entries (they fill a row, in position order); equal values tie even when their NW
 * codes differ (selection on da_nw_code_ranks, as in the two-set form).
 *   idx_out : [n][top] int32, 0-based;  val_out : [n][top] float64 or NULL, val[i][t] bit for bit S[i][idx[i][t]];
 *   diag_out (NW only, may be NULL): [n] float64, S[i][i] as the DP gives it (the MinHash diagonal is 1.0 by the reference's forced diagonal).
 * This is NOT da_similarity_*_cross_topk(x, x, top + 1) with the first column dropped: among byte-identical or equally similar sequences a
 * row's own column is not the first of its ties.  Byte-identical strings fill each other's lists at 1.0: pass distinct sequences.
 * Validation, before any device is needed.  MinHash: what da_similarity_mh checks, in its order and with its texts (n, k, n_hash, NULL pointers,
 * offsets); then n < 2 -> DA_ERR_BAD_ARG ("a nearest neighbour needs a second sequence"); top < 1 or top > n - 1 -> DA_ERR_BAD_ARG; top > 1024 ->
 * DA_ERR_UNSUPPORTED; n_hash > 65535 -> DA_ERR_UNSUPPORTED.  NW: the order of da_similarity_nw_edges -- matrix name, NULL pointers, n < 2 and
 * `top` (where that call checks thresh_p), offsets, residues, then every sequence has 1 .. 127 residues (DA_ERR_UNSUPPORTED).  `top` is not clamped.
 * Route: K1 and the planes once on the n sequences (no joint operand, no padding rows), the square problem's rows [b0, b1) x columns [0, n) as
 * uint16 codes in row blocks of DYNAALIGN_BLOCK_BYTES, and da_dev_topk_rows_self on each block with self_col0 = b0.  NW: on one code buffer pair
 * (p, q) is calc(seq[min(p, q)], seq[max(p, q)]), so those rows are rows of the mirrored square matrix.  Single device, the direct route only. */
int da_similarity_mh_knn(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, int n_hash, const uint32_t *seeds, int top,
                         int32_t *idx_out, double *val_out);
int da_similarity_nw_knn(const uint8_t *residues, const int64_t *offsets, int64_t n, const char *matrix_name, int gap_open, int gap_ext,
                         int top, int32_t *idx_out, double *val_out, double *diag_out);

/* ---- the EXACT Jaccard index of k-shingle sets: what similarityMH estimates, without hash functions, seed or estimator noise ----
 * S_k(s) is the set of distinct length-k byte substrings of s -- byte-wise, any byte value, as the k-mers of da_similarity_mh; empty when
 * len(s) < k.  J(a, b) = (double)|S_k(a) n S_k(b)| / (double)|S_k(a) u S_k(b)|, one IEEE divide of the two integers; 1.0 when both sets are
 * empty (what da_similarity_mh gives two strings shorter than k), 0.0 when exactly one is.  Nothing is forced on the diagonal: J(a, a) is 1.0
 * by the definition.  Empty sequences and sequences shorter than k are legal everywhere; no NaN occurs.
 * uint16 code (DA_OUT_COMPACT): intersection << 8 | union, 0x0101 for two empty sets -- the shape of the NW code, valued by the same divide
 * (a code's low byte is never 0).  Wherever an order is needed (top-k, nearest neighbours, the quantile) equal VALUES tie whatever their
 * codes (2/4 and 3/6): the selection runs on da_nw_code_ranks(127, ...), whose domain holds every (intersection, union) the limits allow.
 * Limits (DA_ERR_UNSUPPORTED, the text names the limit and, for a sequence, its 1-based index): k <= 8 -- the k bytes pack big-endian into one
 * key, 32 bits for k <= 4, 64 bits otherwise -- and every sequence has at most 127 shingle positions, len - k + 1 <= 127, so that the union of
 * a pair fits the code's low byte.
 * Validation, before any device is needed.  One set: n <= 0 -> DA_ERR_EMPTY_INPUT, k <= 0 -> DA_ERR_BAD_K (the texts of da_similarity_mh), NULL
 * pointers, the offsets, k > 8, the sequence lengths; then what the call adds -- _knn: n < 2, top < 1 or top > n - 1 -> DA_ERR_BAD_ARG, top > 1024
 * -> DA_ERR_UNSUPPORTED (the texts of da_similarity_mh_knn); _edges: n < 2, thresh_p outside [0, 1] -> DA_ERR_BAD_ARG (the texts of
 * da_similarity_nw_edges).  Two sets: k <= 0 -> DA_ERR_BAD_K; m <= 0 or n <= 0 returns DA_OK and writes nothing (_cross_topk: m <= 0 returns DA_OK,
 * n <= 0 with m > 0 is DA_ERR_BAD_ARG, no top satisfies 1 <= top <= 0); NULL pointers, the offsets of x then y, k > 8, the lengths of x then y;
 * then top < 1 or top > n -> DA_ERR_BAD_ARG, top > 1024 -> DA_ERR_UNSUPPORTED (the texts of da_similarity_nw_cross_topk).
 *   da_similarity_jaccard             out: n * n doubles.  The device writes uint16 codes, a quarter of the bytes cross PCIe and the host widens them.
 *   da_similarity_jaccard_cross       out: m x n, bit for bit the block [0:m, m:m+n] of da_similarity_jaccard on c(x, y); column_major as
 *                                     da_similarity_mh_cross.  Both sets form ONE set operand [x ; y] on the device.
 *   da_similarity_jaccard_cross_topk  idx_out [m][top] int32, val_out [m][top] float64 or NULL: numpy's argsort(-R, axis = 1, kind = "stable")[:, :top].
 *   da_similarity_jaccard_knn         idx_out / val_out [n][top]: the `top` columns j != i of every row, as da_similarity_mh_knn.  Byte-identical
 *                                     strings (and any two strings with equal shingle sets) fill each other's lists at 1.0.
 *   da_similarity_jaccard_edges[_begin]  threshold = R's type-7 quantile of the strict upper triangle at thresh_p; the edges i <= j, diagonal
 *                                     included, with J >= threshold and J > 0, sorted by (i, j); calling conventions of da_similarity_nw_edges[_begin].
 * Single device, the direct route only; top-k / kNN work in row blocks of DYNAALIGN_BLOCK_BYTES. */
int da_similarity_jaccard(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, double *out);
int da_similarity_jaccard_cross(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m,
                                const uint8_t *y_residues, const int64_t *y_offsets, int64_t n, int k, double *out, int column_major);
int da_similarity_jaccard_cross_topk(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m,
                                     const uint8_t *y_residues, const int64_t *y_offsets, int64_t n, int k, int top, int32_t *idx_out, double *val_out);
int da_similarity_jaccard_knn(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, int top, int32_t *idx_out, double *val_out);
/* (da_similarity_jaccard_edges[_begin] are declared with the other edge-list calls, after da_edges) */
/* The device layer.  da_dev_jaccard_sets: per sequence the ascending distinct keys of its shingles (uint32 for k <= 4, uint64 for k 5 .. 8; the k
 * bytes big-endian) at d_keys[i * ld_keys + 0 .. d_counts[i]) and their number d_counts[i] (uint8); the slots from the count to ld_keys are zeroed
 * and mean nothing -- FF FF FF FF is a legal shingle, the counts say where a list ends.  ld_keys >= da_dev_jaccard_sets_ld(max_len, k), the call's
 * largest shingle count rounded up to a multiple of 4 (at least 4, at most 128): a set of 12-mers at k = 2 costs 12 keys a row.  max_len: the longest
 * sequence (max_len - k + 1 <= 127).  n <= 0 -> DA_ERR_EMPTY_INPUT, k <= 0 -> DA_ERR_BAD_K, NULL pointers -> DA_ERR_BAD_ARG, k > 8 or too long ->
 * DA_ERR_UNSUPPORTED, ld_keys too small -> DA_ERR_BAD_ARG.
 * da_dev_jaccard_rect: rows [row_begin, row_end) x columns [col_begin, col_end) of the n sets, element (i, j) = J(set i, set j), as DA_OUT_COMPACT
 * codes or DA_OUT_F64 doubles at d_out[(i - row_begin) * ld + (j - col_begin)]; any ld >= columns and any naturally aligned d_out (16-byte stores
 * where the address allows, single elements otherwise); every element written once, nothing else touched; an empty rectangle is DA_OK.  Two sets are
 * compared through the sets of their concatenation.  Both calls are asynchronous on `stream`. */
int64_t da_dev_jaccard_sets_ld(int64_t max_len, int k);
int da_dev_jaccard_sets(const uint8_t *d_residues, const int64_t *d_offsets, int64_t n, int64_t max_len, int k, void *d_keys, int64_t ld_keys,
                        uint8_t *d_counts, void *stream);
int da_dev_jaccard_rect(const void *d_keys, const uint8_t *d_counts, int64_t n, int64_t ld_keys, int k, int64_t row_begin, int64_t row_end,
                        int64_t col_begin, int64_t col_end, int kind, void *d_out, int64_t ld, void *stream);

/* ---- the alignment PATH of listed pairs: how x[i] and y[j] align, not only how similar they are ----
 * Pair p aligns x[pair_x[p]] as sequence1 (length m1) with y[pair_y[p]] as sequence2 (length n2); pair_x == pair_y == NULL means p with p
 * (then m == n == pairs).  The fill is the reference's (src/pairwiseSeqAlign.cpp:216-281); the decision of cell (i, j), i, j >= 1, is
 *   D if d >= Ix && d >= Iy (d the diagonal candidate), else U if Ix >= Iy, else L   (:271-279; M[i][j] is overwritten by the winner),
 * border cells (i, 0) are U and (0, j) are L (:228, :234).  The path starts at (m1, n2) and follows the decisions to (0, 0) -- D to (i-1, j-1),
 * U to (i-1, j), L to (i, j-1), the reference's traceback (:284-308) -- and is returned in FORWARD order, from (0, 0) to (m1, n2), over the
 * bytes 'D', 'U', 'L': D puts sequence1[i-1] opposite sequence2[j-1], U puts sequence1[i-1] opposite a gap, L a gap opposite sequence2[j-1].
 *   ops_out     : [pairs][ld_ops] bytes or NULL; row p holds the path of pair p, bytes past its length are 0
 *   len_out     : the path's length = the reference's alignment_length          matches_out : its D steps with equal residues = `matches`
 *   score_out   : M[m1][n2] after the fill (INT32_MIN / 2 when exactly one sequence is empty, 0 when both are)
 * (each [pairs] int32, any may be NULL).  matches / length are the two operands of similarityNW's divide for calc(x[i], y[j]).
 * Empty sequences are legal: an all-L or all-U path; length 0 when both are empty.
 * Validation, before any device is needed, in this order: the matrix name (DA_ERR_BAD_MATRIX); pairs == 0 returns DA_OK and writes
 * nothing; one NULL and one non-NULL list, the NULL form with m != pairs or n != pairs, an index outside [0, m) / [0, n) -> DA_ERR_BAD_ARG;
 * a listed sequence of more than 127 residues -> DA_ERR_UNSUPPORTED; ops_out != NULL with ld_ops smaller than the largest
 * len(x) + len(y) over the listed pairs -> DA_ERR_BAD_ARG; then the residue error the reference's lazy fill would raise first with the pairs
 * visited p ascending, each pair in calc's own order (seq1[0], every character of seq2, seq1[1], ...: an empty sequence1 checks nothing, an
 * empty sequence2 still has sequence1 checked; only listed sequences are checked); then DA_ERR_NO_DEVICE.
 * The device keeps 2 decision bits per cell plus a strip boundary per row in a workspace of da_nw_align_workspace_bytes(pairs) bytes (5 KiB
 * per pair, in whole wavefronts of 64 pairs); the host call works in blocks of pairs whose workspace and ops bytes fit DYNAALIGN_BLOCK_BYTES
 * (half of the free device memory without it; at most 2^19 pairs).  Single device. */
int da_nw_align_pairs(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m,
                      const uint8_t *y_residues, const int64_t *y_offsets, int64_t n,
                      const int32_t *pair_x, const int32_t *pair_y, int64_t pairs,
                      const char *matrix_name, int gap_open, int gap_ext,
                      uint8_t *ops_out, int64_t ld_ops,
                      int32_t *len_out, int32_t *matches_out, int32_t *score_out);
size_t da_nw_align_workspace_bytes(int64_t pairs);
/* The same on device pointers, asynchronous on `stream`: codes and offsets of x and y as da_dev_nw_encode leaves them (the two sets may be the
 * same buffers), device pair lists or NULL, device outputs as above (the ops rows are cleared first).  d_work: at least
 * da_nw_align_workspace_bytes(64) bytes; a workspace smaller than da_nw_align_workspace_bytes(pairs) is reused by consecutive launches of as
 * many pairs as it holds.  The lists live on the device, so nothing is validated against them here: a pair the kernel cannot take (an index
 * outside its set, a sequence of more than 127 residues, ld_ops < len(x) + len(y)) gets length -1, matches -1, score 0 and an empty ops row. */
int da_dev_nw_align_pairs(const uint8_t *d_x_codes, const int64_t *d_x_offsets, int64_t m,
                          const uint8_t *d_y_codes, const int64_t *d_y_offsets, int64_t n,
                          const int32_t *d_pair_x, const int32_t *d_pair_y, int64_t pairs,
                          int matrix_id, int gap_open, int gap_ext,
                          uint8_t *d_ops, int64_t ld_ops, int32_t *d_len, int32_t *d_matches, int32_t *d_score,
                          void *d_work, size_t work_bytes, void *stream);

/* ---- the same for sequences of up to 1024 residues: one wavefront per pair (nw_align_long_kernels.hip) ----
 * da_nw_align_long_pairs has the contract of da_nw_align_pairs, word for word -- arguments, outputs, the validation order and its texts, the
 * reference's lazy residue error, pairs == 0, the NULL-list form, the ld_ops check, DA_ERR_NO_DEVICE last -- with one change: the length
 * refusal (DA_ERR_UNSUPPORTED) is for a listed sequence of more than 1024 residues.  Listed pairs with both sequences of at most 127 residues run
 * through the lane-per-pair kernels of da_nw_align_pairs, every other pair through k_nw_align_long; results come back in listed order.  The
 * host call works in blocks of pairs whose ops rows fit DYNAALIGN_BLOCK_BYTES (half of the free device memory without it).  Single device.
 * k_nw_align_long: the fill is the anti-diagonal sweep of the similarity kernel for 65 .. 1024 residues (lane l owns W columns of sequence2,
 * W the smallest of 1, 2, 3, 4, 6, 8, 9, 12, 16 with 64 W >= len(sequence2)); length, matches and score come out of its (matches, length)
 * payload.  With ops it also stores one 32-bit word of 2-bit decisions per lane and step, [step][lane], into the wave's SLOT of
 * (max_len + 63) * 256 bytes and then walks the pair back itself through a window of steps in LDS.  The grid is persistent: wave s takes pairs
 * s, s + slots, ... and reuses slot s, so the workspace does not grow with the number of pairs. */
int da_nw_align_long_pairs(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m,
                           const uint8_t *y_residues, const int64_t *y_offsets, int64_t n,
                           const int32_t *pair_x, const int32_t *pair_y, int64_t pairs,
                           const char *matrix_name, int gap_open, int gap_ext,
                           uint8_t *ops_out, int64_t ld_ops,
                           int32_t *len_out, int32_t *matches_out, int32_t *score_out);
/* Bytes for min(pairs, 3072) slots of sequences up to max_len (clamped to 1024) residues: 3072 is the number of wavefronts resident on one
 * device.  0 for pairs <= 0 or max_len < 0.  Needs no device. */
size_t da_nw_align_long_workspace_bytes(int64_t pairs, int64_t max_len);
/* On device pointers, asynchronous on `stream`, arguments as da_dev_nw_align_pairs plus max_len, which sizes the slots.  The lists live on
 * the device, so EVERY pair goes through the wavefront-per-pair kernel, short ones included.  With d_ops, d_work must hold at least one slot
 * ((max_len + 63) * 256 bytes, max_len clamped to 1024), else DA_ERR_BAD_ARG; a workspace smaller than
 * da_nw_align_long_workspace_bytes(pairs, max_len) only means fewer wavefronts in flight.  With d_ops == NULL no decision is stored, no walk
 * runs and d_work may be NULL.  A pair the kernel cannot take (an index outside its set, a sequence over max_len or over 1024 residues,
 * ld_ops < len(x) + len(y)) gets length -1, matches -1, score 0 and an empty ops row. */
int da_dev_nw_align_long_pairs(const uint8_t *d_x_codes, const int64_t *d_x_offsets, int64_t m,
                               const uint8_t *d_y_codes, const int64_t *d_y_offsets, int64_t n,
                               const int32_t *d_pair_x, const int32_t *d_pair_y, int64_t pairs,
                               int matrix_id, int gap_open, int gap_ext,
                               uint8_t *d_ops, int64_t ld_ops, int32_t *d_len, int32_t *d_matches, int32_t *d_score,
                               int64_t max_len, void *d_work, size_t work_bytes, void *stream);

/* ---- one consensus sequence per cluster: the center-star consensus on the alignments above (consensus_kernels.hip) ----
 * For a cluster with members s_0 .. s_{c-1} (input order, duplicates kept): c == 1 gives the member itself, copied through unvalidated; otherwise
 * the CENTER is the member i with the largest correctly rounded sum over j != i of matches(i, j) / length(i, j) of the alignments of s_i as
 * sequence1 with s_j (two empty strings count 0.0; ties to the lowest i) -- math.fsum of the doubles, reproduced as an exact 63-bit fixed-point
 * sum in two 64-bit limbs rounded to 53 bits, ties to even, before comparing.  The center is then aligned as sequence1 with every other member;
 * column p of the tally holds the center's residue once and, per other member, the residue a D step puts opposite p or '-' for a U step (L steps
 * are ignored).  The most frequent symbol wins; among tied symbols the center's residue if it is one of them, otherwise the earliest in
 * "ARNDCQEGHILKMFPSTWYVBZX*-"; columns won by '-' are dropped.
 *   cluster_of   : [n] int32, the cluster of every sequence, 0 .. clusters - 1
 *   cons_out     : [clusters][ld_cons] bytes, row k the consensus of cluster k as letters, 0 past its length
 *   cons_len_out : [clusters] int32         center_out : [clusters] int32 or NULL, the input index of each cluster's center
 * Validation, before any device is needed, in this order: the matrix name (DA_ERR_BAD_MATRIX); n == clusters == 0 returns DA_OK; negative counts,
 * NULL pointers, the offsets, a cluster_of outside its range, a cluster without a member -> DA_ERR_BAD_ARG; a member of more than 1024 residues in a
 * cluster of two or more -> DA_ERR_UNSUPPORTED, in the words of da_nw_align_long_pairs; ld_cons smaller than the longest member -> DA_ERR_BAD_ARG;
 * then the residue error da_nw_align_long_pairs raises first on all ordered pairs of all clusters of two or more (clusters ascending, i ascending,
 * j != i ascending, each pair in calc's lazy order as above), derived from every member's first bad position; then DA_ERR_NO_DEVICE (not when every
 * cluster has one member).  If every member of a cluster of two or more has at most 127 residues the lane-per-pair kernels align, otherwise every
 * pair takes a wavefront; the result is the same.  Both phases work in blocks within DYNAALIGN_BLOCK_BYTES (half of the free device memory
 * without it).  Single device. */
int da_cluster_consensus(const uint8_t *residues, const int64_t *offsets, int64_t n, const int32_t *cluster_of, int64_t clusters,
                         const char *matrix_name, int gap_open, int gap_ext, uint8_t *cons_out, int64_t ld_cons, int32_t *cons_len_out,
                         int32_t *center_out);
/* On device pointers, asynchronous on `stream`, nothing returning to the host between the phases.  The n sequences (codes and offsets as
 * da_dev_nw_encode leaves them, all residues valid) are POOLED: cluster k is sequences cluster_ptr[k] .. cluster_ptr[k + 1] - 1, at least one each,
 * cluster_ptr[0] == 0 and cluster_ptr[clusters] == n.  The table is given twice: cluster_ptr on the host, which plans the blocks and is read only
 * during the call, and d_cluster_ptr, the same int64 values on the device, which the kernels read.  max_len: the longest sequence (<= 1024, else
 * DA_ERR_UNSUPPORTED; <= 127 selects the lane-per-pair kernels).  d_cons [clusters][ld_cons] (ld_cons >= max_len; bytes past a row's length are
 * not written), d_cons_len [clusters], d_center [clusters]: the center as a pooled index.  d_work: da_dev_cluster_consensus_workspace_bytes(...,
 * minimal = 1) bytes at least (blocks of 64 pairs), with minimal = 0 what the largest blocks take (at most 2^20 pairs or rows each); anything in
 * between means smaller blocks.  Phase 1 cuts its blocks of pairs anywhere; phase 2 takes groups of whole clusters, and a cluster with more rows
 * than a block holds alone, in member chunks, its tally carried in the workspace. */
size_t da_dev_cluster_consensus_workspace_bytes(const int64_t *cluster_ptr, int64_t clusters, int64_t max_len, int minimal);
int da_dev_cluster_consensus(const uint8_t *d_codes, const int64_t *d_offsets, int64_t n, const int64_t *cluster_ptr, const int64_t *d_cluster_ptr,
                             int64_t clusters, int64_t max_len, int matrix_id, int gap_open, int gap_ext, uint8_t *d_cons, int64_t ld_cons,
                             int32_t *d_cons_len, int32_t *d_center, void *d_work, size_t work_bytes, void *stream);
/* The pieces.  PAIRS are numbered per cluster i ascending then j != i ascending, cluster k from the running sum of c (c - 1); ROWS are
 * (center, j != center), j ascending, cluster k from cluster_ptr[k] - k.
 * da_dev_consensus_center_sums: d_len / d_matches hold the results of pairs [pair_begin, pair_begin + pairs) (entry 0 is pair_begin); every term
 * matches / length (0 when length <= 0) is ADDED as 63-bit fixed point to its member's two limbs d_sums[2 g], d_sums[2 g + 1] (low, high; the
 * caller clears them first).  Consecutive calls may cut the pairs anywhere.  d_pair_ptr: [clusters + 1] int64 of scratch the call fills.
 * da_dev_consensus_pick: d_center[k] = the pooled index of the member of cluster k whose sum, rounded to 53 bits ties to even, is largest (the
 * lowest among equals).
 * da_dev_consensus_vote: for clusters [cluster_begin, cluster_begin + cluster_count), one workgroup each, the ops rows [row_begin, row_begin + rows)
 * at d_ops (row_begin first; d_len their lengths, or NULL: a row ends at its first 0 byte or at ld_ops).  A cluster whose rows all lie in the range
 * gets its consensus row and length; one that starts before it takes its tally from d_carry (25 * len(center) uint32), one that goes on past it
 * leaves it there. */
int da_dev_consensus_center_sums(const int32_t *d_len, const int32_t *d_matches, int64_t pair_begin, int64_t pairs, const int64_t *cluster_ptr,
                                 const int64_t *d_cluster_ptr, int64_t clusters, int64_t *d_pair_ptr, uint64_t *d_sums, void *stream);
int da_dev_consensus_pick(const uint64_t *d_sums, const int64_t *d_cluster_ptr, int64_t clusters, int32_t *d_center, void *stream);
int da_dev_consensus_vote(const uint8_t *d_codes, const int64_t *d_offsets, const int64_t *d_cluster_ptr, const int32_t *d_center,
                          int64_t cluster_begin, int64_t cluster_count, const uint8_t *d_ops, int64_t ld_ops, const int32_t *d_len, int64_t row_begin,
                          int64_t rows, uint32_t *d_carry, uint8_t *d_cons, int64_t ld_cons, int32_t *d_cons_len, int64_t max_len, void *stream);

/* ---- device-pointer entry points (bench / multi-GPU sharding) ------------ */

/* Leading dimension (in uint32 elements) the library uses for signature
 * matrices: n_hash rounded up to a multiple of 32. */
int64_t da_sig_ld(int n_hash);

/* K1: signature build.
 *   d_sig : n rows of ld_sig (>= n_hash) uint32 -- the signatures themselves
 *           (src/minHash.cpp:140-157); columns [n_hash, ld_sig) not written. */
int da_dev_minhash_signatures(const uint8_t *d_residues, const int64_t *d_offsets, int64_t n,
                              int64_t total_residues, int64_t max_len,
                              int k, int n_hash, const uint32_t *d_seeds,
                              uint32_t *d_sig, int64_t ld_sig, void *stream);

/* K1b: signatures -> operand of the compare kernel.  The compare only asks "equal or not" per
 * hash function (src/minHash.cpp:168-173), so each column of d_sig is re-coded exactly: values
 * occurring >= 2 times get dense ids, values occurring once get codes that never match (one code
 * on the row side, another on the column side; the compare kernel forces the diagonal).  The
 * codes are then bit-transposed per group of 32 hash functions with as many bit planes as the
 * largest column dictionary needs -- 8, 12 or 16 instead of the 32 of the raw values -- and the
 * bit-sliced compare does that fraction of the work.  Exact for every input with n <= 131068
 * (at most n/2 repeated values per column fit 16 bits); larger n -- or the never-observed
 * overflow of the dictionary's LDS table -- produce the raw 32-plane operand instead.
 *   min_plane_bits: 0 = as few planes as the data needs; 12 / 14 / 15 / 16 = at least that many code
 *                   bits; 32 = raw signature bits (no dictionary).  (14 / 15 = the 16-plane operand with
 *                   its top planes zero: the hand-scheduled kernel skips their step / half step.)
 *   d_planes      : 16-byte aligned buffer of planes_words >= da_mh_planes_words(n, n_hash)
 *                   uint32; opaque (blocked in the order the compare kernel stages it).
 *   d_work        : da_mh_planes_workspace_bytes(n, n_hash) bytes of scratch, 256-byte aligned
 *   plane_bits_out: 8, 12, 14, 15, 16 or 32 -- pass it to da_dev_mh_compare[_shard].
 * Synchronises `stream` once (reads the dictionary's status words) on the dictionary route.
 * The environment variable DYNAALIGN_PLANE_BITS (12, 16, 32) raises min_plane_bits (debugging aid;
 * it also reaches the host-pointer entry points). */
int64_t da_mh_planes_words(int64_t n, int n_hash);
size_t da_mh_planes_workspace_bytes(int64_t n, int n_hash);
int da_dev_mh_planes(const uint32_t *d_sig, int64_t ld_sig, int64_t n, int n_hash, int min_plane_bits,
                     void *d_work, size_t work_bytes, uint32_t *d_planes, int64_t planes_words,
                     int *plane_bits_out, void *stream);

/* K2: all-pairs signature compare (bit-sliced: OR over planes of a XOR b, then
 * popcount; matches = n_hash - mismatches).
 * Computes rows [row_begin,row_end) of the n x n result into d_out, which
 * holds (row_end-row_begin) rows of leading dimension ld (>= n) elements.
 *   symmetric != 0 : requires row_begin == 0, row_end == n; only tiles on or
 *                    above the diagonal are compared and each is stored twice
 *                    (direct + mirrored), like src/minHash.cpp:175-176.
 *   symmetric == 0 : every (i,j) of the row block is compared (row-sharding).
 * kind selects double or uint16 counts.  Diagonal = 1.0 / n_hash.
 * d_planes, plane_bits: from da_dev_mh_planes for the same n and n_hash. */
int da_dev_mh_compare(const uint32_t *d_planes, int plane_bits, int64_t n, int n_hash,
                      int64_t row_begin, int64_t row_end, int symmetric,
                      int kind, void *d_out, int64_t ld, void *stream);

/* K2 on a RECTANGLE: rows [row_begin, row_end) x columns [col_begin, col_end) of the n-row problem the planes were built for, every element
 * stored once: d_out holds (row_end - row_begin) rows of ld >= col_end - col_begin elements, element (i, j) at
 * d_out[(i - row_begin) * ld + (j - col_begin)].  The row-block mode of da_dev_mh_compare is col_begin = 0, col_end = n.  An element whose
 * global row equals its global column is n_hash (1.0), as there; everything else is a plain pair, so two sets compared through one
 * operand must have been coded by ONE da_dev_mh_planes call on their concatenation.  kind = DA_OUT_F64 or DA_OUT_COMPACT.
 * The hand-scheduled 12- and 14 / 15 / 16-bit loops take every tile that lies wholly inside the rectangle and off the global diagonal when
 * row_begin and col_begin are multiples of 128, ld is even and d_out is 16-byte (float64; n_hash <= 4607 / 5119) or 4-byte (uint16) aligned;
 * the compiled kernel takes the rest, or everything (8 / 32 planes, odd ld, unaligned output or origins, DYNAALIGN_K2_NO_ASM=1). */
int da_dev_mh_compare_rect(const uint32_t *d_planes, int plane_bits, int64_t n, int n_hash,
                           int64_t row_begin, int64_t row_end, int64_t col_begin, int64_t col_end,
                           int kind, void *d_out, int64_t ld, void *stream);

/* similarityMH_cross (see da_similarity_mh_cross) on two resident sets as ONE call, like da_dev_similarity_mh: d_out = m rows of ld >= n
 * doubles.  Direct route: K1 per side into one signature matrix [x ; filler ; y] (x padded to a multiple of 128 rows with rows that repeat
 * real ones: every equality is kept, their results are never stored), K1b ONCE on the union, da_dev_mh_compare_rect's kernels.  Duplicate
 * route: byte-identical strings are collapsed PER SIDE (U_x, U_y unique strings), the unique strings are compared into a U_x x U_y uint16
 * table and a rectangular row expansion (a workgroup holds a table row in LDS and writes the output rows of its copies in x, columns through
 * y's id map) writes every element once.  Taken when sqrt(U_x U_y / (m n)) <= 0.68 (DYNAALIGN_MH_DEDUP_MAX_PCT, in percent), m + n >= 2048
 * (DYNAALIGN_MH_DEDUP_MIN_N), U_y <= 65536, n_hash <= 2047, ld even and d_out 16-byte aligned; DYNAALIGN_MH_NO_DEDUP=1 disables it.
 * One stream; no pipelining, packed table, heavy / rare split or sparse route here.  n_hash <= 65535.  Synchronises the stream.
 * da_mh_cross_last_route: what the calling thread's last such call did -- m, n, unique strings per side (m, n when no plan was made),
 * route (0 direct, 1 duplicate), the plane count K1b chose and the times in ms of {plans, K1 + K1b, K2, copy lists, expansion}
 * (direct: {plans, K1 + K1b, K2, 0, 0}).  Any pointer may be NULL. */
int da_dev_similarity_mh_cross(const uint8_t *d_x_residues, const int64_t *d_x_offsets, int64_t m, int64_t x_total,
                               const uint8_t *d_y_residues, const int64_t *d_y_offsets, int64_t n, int64_t y_total,
                               int k, int n_hash, const uint32_t *d_seeds, double *d_out, int64_t ld, void *stream);
int da_mh_cross_last_route(int64_t *m_out, int64_t *n_out, int64_t *unique_x_out, int64_t *unique_y_out, int *route_out,
                           int *plane_bits_out, double *ms5_out);

/* Exact top-k selection per row of a block of uint16 keys: d_keys holds `rows` rows of ld >= n keys.  A key's order is its rank,
 * d_rank[key] (a 65536-entry table) or the key itself when d_rank is NULL; every rank must be < 2^rank_bits (rank_bits 1 .. 16, 0 = 16:
 * it only places the two 8-bit digits of the radix select; ranks beyond it give a wrong selection, never an access out of bounds).
 * For every row: d_idx[row * ld_out + t], d_key_out[row * ld_out + t], t < top, are the column and the KEY of the t-th element in
 * (rank descending, column ascending) order -- argsort(-rank[row], kind = "stable")[:top].  1 <= top <= n; top > 1024 is
 * DA_ERR_UNSUPPORTED (the candidates of a row are sorted in a fixed LDS buffer); ld_out >= top.  One workgroup per row, the row is never
 * sorted: a two-level radix select finds the rank of the top-th element, an ordered compaction keeps what lies above it and the first
 * columns equal to it, and only those <= top candidates are sorted.  Rows are read in 16-byte units where their address allows it,
 * in 2-byte units otherwise: every ld and base address works.  Asynchronous on `stream`. */
int da_dev_topk_rows(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, const uint16_t *d_rank, int rank_bits, int top,
                     int32_t *d_idx, uint16_t *d_key_out, int64_t ld_out, void *stream);

/* similarityMH_cross followed by the per-row top-k selection (see da_similarity_mh_cross_topk) on two resident sets as ONE call:
 * d_idx (int32) and d_val (float64) hold m rows of ld_out >= top elements.  The operand is da_dev_similarity_mh_cross's
 * ([x ; filler ; y], same padding and 131 068-row rule); per row block of x, sized from DYNAALIGN_BLOCK_BYTES by the column count alone:
 * the rectangle compare into uint16 counts, da_dev_topk_rows, the selected counts divided by n_hash.  Direct route only (no duplicate
 * collapse, packed table, heavy / rare split or sparse route); n_hash <= 65535; one stream, which it synchronises. */
int da_dev_similarity_mh_cross_topk(const uint8_t *d_x_residues, const int64_t *d_x_offsets, int64_t m,
                                    const uint8_t *d_y_residues, const int64_t *d_y_offsets, int64_t n,
                                    int k, int n_hash, const uint32_t *d_seeds, int top, int32_t *d_idx, double *d_val, int64_t ld_out,
                                    void *stream);

/* da_dev_topk_rows with every row's own column left out of the selection: the block is rows [self_col0, self_col0 + rows) of a square problem,
 * so its row r owns column self_col0 + r, and that element is absent from the radix select, from the ordered compaction and from the choice
 * among equals -- the result is argsort(-rank[row], kind = "stable")[:top] of the row without it.  d_self_key (may be NULL): uint16[rows], receives
 * the key found at the own column (the NW diagonal).  A row whose own column falls outside [0, n) excludes nothing and leaves its d_self_key
 * entry unwritten.  1 <= top <= n - 1 (DA_ERR_BAD_ARG); everything else as da_dev_topk_rows. */
int da_dev_topk_rows_self(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, const uint16_t *d_rank, int rank_bits, int top,
                          int64_t self_col0, int32_t *d_idx, uint16_t *d_key_out, int64_t ld_out, uint16_t *d_self_key, void *stream);

/* da_similarity_mh_knn on a resident set as ONE call: d_idx (int32) and d_val (float64) hold n rows of ld_out >= top elements.  Validates like
 * da_similarity_mh_knn (n, k, n_hash, NULL pointers, n < 2, top, n_hash > 65535, ld_out) before it touches the device; one stream, which it
 * synchronises. */
int da_dev_similarity_mh_knn(const uint8_t *d_residues, const int64_t *d_offsets, int64_t n, int k, int n_hash, const uint32_t *d_seeds,
                             int top, int32_t *d_idx, double *d_val, int64_t ld_out, void *stream);

/* Nearest-neighbour lists -> the edge list of their kNN graph, on the device.  d_idx / d_key: n rows of ld >= top entries (top <= 1024), row r
 * listing r's neighbours and the uint16 keys found there (what da_dev_topk_rows_self wrote).  An entry (r -> j) is live when its key stands for
 * a value > 0: key != 0, or key >> 8 != 0 with is_nw (the convention of da_dev_widen).  in(i, j): j appears live in row i.
 *   mode DA_KNN_UNION keeps the pair {i, j} when in(i, j) or in(j, i); DA_KNN_MUTUAL when both hold.
 * Output: (d_i[e] <= d_j[e], d_v[e]) -- the key of the entry that produced it -- and *d_count (uint64) = the number of entries, in the form
 * da_dev_edges_to_csr takes.  With `loops` every vertex r also gets (r, r, d_self_key[r]), or (r, r, self_code) when d_self_key is NULL (MinHash:
 * n_hash).  d_i / d_j / d_v must hold n * (top + (loops ? 1 : 0)) entries.  One wave per source row; every pair is emitted by exactly one row
 * (union: row min(i, j) when in(min, max), else row max; mutual: row min), at a position given by a count pass and an exclusive scan -- no output
 * atomic, so the list depends on the data alone.  It is grouped by emitting row, not sorted by (i, j).  The membership test scans row j's entries;
 * it does not rely on the lists being symmetric.  d_work: da_dev_knn_edges_bytes(n, top) bytes, 256-byte aligned.  Asynchronous on `stream`. */
#define DA_KNN_UNION 0
#define DA_KNN_MUTUAL 1
size_t da_dev_knn_edges_bytes(int64_t n, int top);
int da_dev_knn_edges(const int32_t *d_idx, const uint16_t *d_key, int64_t ld, int64_t n, int top, int mode, int is_nw,
                     const uint16_t *d_self_key, int self_code, int loops, void *d_work, size_t work_bytes, int32_t *d_i, int32_t *d_j,
                     uint16_t *d_v, uint64_t *d_count, void *stream);

/* K1 + K1b + K2 as ONE call: similarityMH (src/minHash.cpp:119-188) from packed residues in HBM to the dense float64
 * n x n matrix in HBM (d_out, leading dimension ld >= n doubles; 16-byte aligned and even ld for the wide-store kernels).
 * Byte-identical sequences have identical signatures, so -- like da_dev_nw -- the call first collapses them: signatures,
 * dictionary codes and the compare run on the U unique strings (K2's work shrinks by (U/n)^2) and the n x n matrix is an
 * index expansion of the U x U count table.  Exact; taken when U <= 0.68 n (0.6 n when only the tile expansion applies; below that K2's saving
 * outweighs the expansion), n >= 2048, U <= 65536, n_hash <= 2047; otherwise the three kernels run on all n rows (what uniform peptides
 * get).  Allocates its intermediates itself (parked between calls, da_release_device_memory frees them) and synchronises
 * the stream.  DYNAALIGN_MH_NO_DEDUP=1 disables the route.  da_mh_last_route reports what the calling thread's last such
 * call did: n, unique strings, whether the route was taken, the plane count K1b chose, and the times in ms of
 * {plan, K1 + K1b, K2, column gather, k_expand_rows, diagonal / border tiles} (direct route: {plan, K1 + K1b, K2, 0, 0, 0}).
 * A second exact route serves inputs without duplicates whose signatures rarely agree (uniform random peptides: 1.4e8 matching
 * (pair, hash function) incidences at n = 100k against 2.5e12 compared ones): the dictionary codes of K1b say which sequences
 * share a value in a column; those incidences are enumerated, bucketed per 128 x 128 output tile, added up in LDS and every tile
 * is written once.  Taken when the input has few duplicates (>= 90 % unique), the incidences number <= n_hash / 5000 per pair on average and
 * <= DYNAALIGN_MH_SPARSE_MAX_PAIRS (default 4e8) in all, no value occurs more than 4096 times in a column, <= 32768 repeated values per column, n >= 2048, n_hash <= 2047; DYNAALIGN_MH_NO_SPARSE=1 disables it.
 * Then *dedup_taken_out = 2, *unique_out = the number of incidences and the times are {plan, K1 + K1b, buckets, 0, tile pass, 0}.
 * The duplicate route's expansion has two kernel families, each with a form PIPELINED with K2 (DYNAALIGN_MH_EXPAND = rowspipe | rows | pipe |
 * tiles picks one; default: the first whose shape test passes; DYNAALIGN_MH_NO_PIPE=1 takes the pipelined forms out):
 *   rows (*dedup_taken_out = 4)   K2 on the table, then ONE pass that holds a table row in LDS and writes the output rows of its copies
 *                                 (16-byte stores: needs an even ld and a 16-byte aligned d_out); times {plan, K1 + K1b, K2, copy lists, that pass, 0}
 *   tiles (= 1)                   K2, column gather, tile expansion + diagonal / border tiles (the times listed above)
 *   rowspipe (= 5), pipe (= 3)    the same kernels with the table compared in bands of 1024 rows by a persistent kernel on a side stream (needs 12
 *                                 code planes and n_hash > 32) while the finished table rows are expanded; unique strings are numbered by first
 *                                 occurrence.  The times are then {plan, K1 + K1b, the compare's span, copy lists (rows) / sum of the gather launches
 *                                 (tiles), time some expansion launch was running, diagonal / border tiles} -- the middle three overlap;
 *                                 da_mh_last_route_chunks gives the number of chunks and of expansion launches.
 * All forms write the same bits.
 * Heavy / rare split (round 4; the direct route; the duplicate route's table compare when its dictionaries need more than 12 planes -- the banded kernel of the
 * pipelined forms exists for 12 and 8 planes -- or with DYNAALIGN_MH_HYBRID_DEDUP=1): when the column
 * dictionaries need 12 - 16 code planes but nearly all matching incidences sit on each column's 254 most frequent values (clustered data: 7e6 of
 * 2.2e10 on the h3n2-like 100k set), the bit-sliced compare runs on EIGHT planes of dense codes for those values -- every other value reads as
 * "never equal" -- and the incidences of the remaining repeated values are enumerated by the sparse route's list kernels and added to the result
 * (count' = count + m, the float64 element recomputed as (count + m) / n_hash: same division, same bits).  Exact.  Taken when 16384
 * (DYNAALIGN_MH_HYBRID_MIN_N) <= n <= 131072, 32 < n_hash <= 2047, <= 32768 repeated values per column, the largest rare class <= 4096, the rare
 * incidences number <= DYNAALIGN_MH_SPARSE_MAX_PAIRS in all and <= n_hash / 25000 per pair on average;
 * DYNAALIGN_MH_NO_HYBRID=1 disables it.  Then *plane_bits_out = 8 and da_mh_last_route_split gives the number of rare incidences (-1: not taken)
 * and the plane count the dictionaries would have needed.
 * Any pointer may be NULL. */
int da_dev_similarity_mh(const uint8_t *d_residues, const int64_t *d_offsets, int64_t n, int64_t total_residues,
                         int k, int n_hash, const uint32_t *d_seeds, double *d_out, int64_t ld, void *stream);
int da_mh_last_route(int64_t *n_out, int64_t *unique_out, int *dedup_taken_out, int *plane_bits_out, double *ms6_out);
int da_mh_last_route_chunks(int *chunks_out, int *expand_launches_out);
int da_mh_last_route_split(int64_t *rare_incidences_out, int *plane_bits_without_out);

/* ---- the pieces of the duplicate-collapsing routes, for callers that orchestrate the steps themselves (the one-process-per-GPU
 * sharded drivers: every rank builds the same plan, computes ITS shard of the unique table with the *_shard / *_unique_rows calls
 * on the plan's strings, all-gathers the shards -- (U/n)^2 of the bytes -- and expands locally).
 * da_dev_unique_plan: byte-identical strings of (d_bytes, d_offsets) collapsed (exact: byte-for-byte compares).  Fills *plan with
 * device pointers INTO d_work (valid while d_work lives): unique id of every input row, first / last occurrence of every unique
 * string, the unique strings back to back + their offsets, and per 64-row block of the unique table the smallest first / largest
 * last occurrence (the ordered NW sweep skips what no original pair i < j needs).  Multi-copy strings are numbered before single-copy
 * ones, each group in input order.  Synchronises `stream` once (the unique count). */
typedef struct da_unique_plan {
  uint32_t struct_size;            /* sizeof(da_unique_plan), set by the caller */
  int32_t reserved;
  int64_t n, unique;
  const int32_t *d_uidx;           /* [n] */
  const int32_t *d_ufirst;         /* [unique] */
  const int32_t *d_ulast;          /* [unique] */
  const uint8_t *d_ubytes;         /* the unique strings */
  const int64_t *d_uoffsets;       /* [unique + 1] */
  const int32_t *d_minfirst;       /* [ceil(unique / 64)] */
  const int32_t *d_maxlast;        /* [ceil(unique / 64)] */
} da_unique_plan;
size_t da_dev_unique_plan_bytes(int64_t n, int64_t total_bytes);
int da_dev_unique_plan(const uint8_t *d_bytes, const int64_t *d_offsets, int64_t n, int64_t total_bytes, void *d_work, size_t work_bytes,
                       da_unique_plan *plan, void *stream);
/* gathered MinHash shards of an n-row problem (da_dev_mh_compare_shard blocks in rank order: value_bits = 0 and ld_g = da_shard_ld, or
 * da_dev_pack_shard blocks: value_bits = their bit count) -> the symmetric uint16 count table [n][ld_table]. */
int da_dev_shards_to_table(const void *d_gathered, int64_t ld_g, int64_t n, int world, int value_bits, uint16_t *d_table, int64_t ld_table,
                           void *stream);
/* rank `rank` of `world`'s part of the ORDERED unique table of similarityNW, calc(U_p, U_q) with U_p as sequence1
 * (src/pairwiseSeqAlign.cpp:340-346 evaluates calc(seq[i], seq[j]) for i < j and the function is not symmetric): the cyclic 128-row
 * units rank, rank + world, ... stored back to back in d_out (ceil(ceil(unique / 128) / world) * 128 rows of ld >= unique uint16
 * matches<<8|length codes; world = 1: the whole table in natural row order).  Every entry some original pair needs -- p == q, or
 * d_ufirst[p] < d_ulast[q] -- is written.  What no pair needs is skipped per row and 64-column tile only (row p against the columns of tile t
 * when d_ufirst[p] >= d_maxlast[t], and never inside a diagonal tile): such an entry either stays unwritten or holds its correct code, so the
 * caller must not read meaning into an unneeded entry either way.  Rows of the last unit past the table stay unwritten.  The plan
 * must have been built on the ENCODED residues (da_dev_nw_encode).  Sequences of 1..64 residues, penalties >= 0. */
int da_dev_nw_unique_rows(const da_unique_plan *plan, int64_t max_len, int matrix_id, int gap_open, int gap_ext, int rank, int world,
                          uint16_t *d_out, int64_t ld, void *stream);
/* the n x n uint16 matrix WITHOUT its duplicate rows: d_rows[r][j] = table[r][u(j)] for every unique string r and every sequence j from
 * the 128-column tile of r's first occurrence on ([unique][ceil8(n)] uint16, da_dev_unique_rows_bytes; natural-row-order table of at most
 * 65536 strings).  Row i of the full matrix is row plan->d_uidx[i] of it for every j >= i: exactly what the *_rows variants of the
 * histogram / edge-extraction calls below read (the threshold + edge list of the duplicate route, with no n x n matrix at all). */
size_t da_dev_unique_rows_bytes(int64_t n, int64_t unique);
int da_dev_unique_rows(const uint16_t *d_table, int64_t ld_table, const da_unique_plan *plan, uint16_t *d_rows, void *stream);
int da_dev_upper_histogram_rows(const uint16_t *d_rows, int64_t ld, const int32_t *d_rowmap, int64_t n, int nbins, uint64_t *d_hist,
                                void *stream);
int da_dev_extract_edges_rows(const uint16_t *d_rows, int64_t ld, const int32_t *d_rowmap, int64_t n, const uint8_t *d_keep, int nbins,
                              int include_diagonal, int32_t *d_i, int32_t *d_j, uint16_t *d_v, int64_t capacity, uint64_t *d_count,
                              void *stream);
/* dense float64 n x n result from the table of the unique strings: out[i][j] = value(table[u(min(i,j))][u(max(i,j))]), value = count / n_hash
 * (is_nw = 0) or matches / length (is_nw = 1, nw_max_len = longest sequence).  table_world = 1: row r of the table is row r; > 1: the
 * table is the all-gathered row blocks of cyclic 128-row units (rank p computed units p, p + world, ...; every block holds
 * ceil(ceil(unique / 128) / world) * 128 rows).  d_work: da_dev_expand_workspace_bytes bytes (the column-gathered twin of the
 * table for the two streaming passes; with less, or NULL, the one-kernel expansion runs).  MinHash tables in one block (is_nw = 0, table_world = 1;
 * the table must be the full symmetric square) with an even ld, a 16-byte aligned d_out, unique <= 65536 and n_hash <= 2047 take the ROW expansion
 * instead (every output row written once from its table row held in LDS; d_work then only holds a few MB of copy lists; DYNAALIGN_EXPAND_NO_STREAM=1
 * keeps the tile passes). */
size_t da_dev_expand_workspace_bytes(int64_t n, int64_t unique, int is_nw, int n_hash, int nw_max_len);
int da_dev_expand_unique(const uint16_t *d_table, int64_t ld_table, int table_world, const da_unique_plan *plan, int is_nw, int n_hash,
                         int nw_max_len, void *d_work, size_t work_bytes, double *d_out, int64_t ld, void *stream);

/* K0: validate + encode residues to BLOSUM row indices 0..23
 * (src/pairwiseSeqAlign.cpp:15-21).  d_codes[total]; *d_bad (int32, caller
 * zeroes it) becomes INT32_MAX - (smallest offending byte position) if any
 * byte is not one of ARNDCQEGHILKMFPSTWYVBZX*, and stays 0 otherwise. */
int da_dev_nw_encode(const uint8_t *d_residues, int64_t total_residues,
                     uint8_t *d_codes, int32_t *d_bad, void *stream);

/* Sequence lengths: <= 64 residues run one lane per pair (k_nw_short), 65..1024 one wavefront per pair (k_nw_long),
 * 1025..32767 the same sweep in column blocks of 1024 with the block boundary spilled to HBM (k_nw_xlong; float64 / 32-bit
 * packed output; synchronises the stream); longer ones fail with DA_ERR_UNSUPPORTED (16-bit alignment length). */
/* K3: all-pairs NW identity.  Same row-block / symmetric / ld conventions as
 * da_dev_mh_compare.  d_codes from da_dev_nw_encode.  kind: double ratio or
 * uint16 (matches<<8|len).  d_score (int32, same shape, ld_score) may be NULL.
 * max_len = longest sequence (host knows it from offsets). */
int da_dev_nw(const uint8_t *d_codes, const int64_t *d_offsets, int64_t n, int64_t max_len,
              int matrix_id, int gap_open, int gap_ext,
              int64_t row_begin, int64_t row_end, int symmetric,
              int kind, void *d_out, int64_t ld, int32_t *d_score, int64_t ld_score,
              void *stream);

/* K3 on a RECTANGLE: the row-block mode of da_dev_nw restricted to the columns [col_begin, col_end); d_out holds (row_end - row_begin) rows of
 * ld >= col_end - col_begin elements.  Pair (i, j) is calc(seq[min(i, j)], seq[max(i, j)]) as everywhere: on the codes of c(x, y), rows of x
 * against columns of y give calc(x[i], y[j]) row-major, rows of y against columns of x the same values column-major.  Direct sweep only (no
 * duplicate route, no prefix sharing); no score output; any kind. */
int da_dev_nw_rect(const uint8_t *d_codes, const int64_t *d_offsets, int64_t n, int64_t max_len,
                   int matrix_id, int gap_open, int gap_ext,
                   int64_t row_begin, int64_t row_end, int64_t col_begin, int64_t col_end,
                   int kind, void *d_out, int64_t ld, void *stream);

/* With symmetric != 0, kind F64 / COMPACT and no score output, da_dev_nw (and da_similarity_nw[_edges]) first collapse
 * byte-identical sequences: the DP runs on the table of unique strings -- as an ORDERED square, calculate_similarity is
 * not symmetric (src/pairwiseSeqAlign.cpp:340-346 evaluates calc(seq[i], seq[j]), i < j) -- and the n x n result is an index
 * expansion of it.  Exact; taken when >= 15 % of the sequences are duplicates, n >= 2048, sequences <= 64 residues,
 * penalties >= 0; synchronises the stream.  DYNAALIGN_NW_NO_DEDUP=1 disables it.  da_nw_last_route reports what the calling
 * thread's last such call did: n, unique strings, whether the route was taken, and {plan, DP kernel, expansion} times in ms
 * (direct route: {0, DP kernel, 0}).  Any pointer may be NULL. */
int da_nw_last_route(int64_t *n_out, int64_t *unique_out, int *dedup_taken_out, double *ms3_out);

/* ---- row-sharding of the pair space over the GPUs of a node ---
 * Rank p of `world` owns the tile rows p, p+world, p+2*world, ... of the pair
 * space (tile = 128 rows for both kinds; cyclic so the upper-triangular work
 * is balanced) and computes only the tiles on or right of the diagonal.  Its
 * result is a compact uint16 block of da_shard_rows() rows x da_shard_ld()
 * columns in a FOLDED layout: local tile rows q and Q-1-q share one stored tile
 * row (the first left-aligned from its diagonal tile, the second right-aligned),
 * which halves the bytes to exchange.  One all-gather of those equally sized
 * blocks (RCCL; rank order) followed by da_dev_finalize_shards on every rank
 * reassembles the full float64 matrix.  The reference has no counterpart (it is
 * single-process); the math per pair is unchanged. */
int64_t da_shard_rows(int64_t n, int world, int is_nw);
int64_t da_shard_ld(int64_t n, int world, int is_nw);
int da_dev_mh_compare_shard(const uint32_t *d_planes, int plane_bits, int64_t n, int n_hash,
                            int rank, int world, uint16_t *d_local, int64_t ld, void *stream);
int da_dev_nw_shard(const uint8_t *d_codes, const int64_t *d_offsets, int64_t n, int64_t max_len,
                    int matrix_id, int gap_open, int gap_ext, int rank, int world,
                    uint16_t *d_local, int64_t ld, void *stream);
/* d_gathered: world * da_shard_rows() rows of ld_g >= da_shard_ld() uint16 (the all-gather output).
 * Writes out[i][j] for all i,j < n: MH count/n_hash, NW (v>>8)/(v&255), mirrored. */
int da_dev_finalize_shards(const uint16_t *d_gathered, int64_t ld_g, int64_t n, int world,
                           int is_nw, int n_hash, double *d_out, int64_t ld_out, void *stream);

/* The MH exchange in value_bits = bits(n_hash) <= 16 bits per count instead of 16 (9 at n_hash = 500;
 * the all-gather is what the multi-GPU MH step waits for): da_dev_pack_shard turns a rank's uint16
 * block into a byte plane (low 8 bits) + value_bits - 8 bit planes, da_shard_packed_bytes() bytes in
 * all, 8-byte aligned; one all-gather of those; da_dev_finalize_shards_packed expands the gathered
 * world * da_shard_packed_bytes() bytes to the dense float64 matrix like da_dev_finalize_shards. */
int64_t da_shard_packed_bytes(int64_t n, int world, int value_bits);
int da_dev_pack_shard(const uint16_t *d_local, int64_t ld, int64_t n, int world, int value_bits,
                      uint8_t *d_packed, void *stream);
int da_dev_finalize_shards_packed(const uint8_t *d_gathered, int64_t n, int world, int value_bits,
                                  int n_hash, double *d_out, int64_t ld_out, void *stream);

/* ---- threshold + sparsify: what clusterbreak does right after sim_fn ---------
 * reference R/clusterbreak.R:219-221 (+ netcluster's graph_from_adjacency_matrix
 * mode = "upper", :122-124):
 *     threshold <- quantile(pep.sim[upper.tri(pep.sim)], thresh_p)      (R type 7)
 *     pep.sim[pep.sim < threshold] <- 0
 * MinHash similarities take n_hash+1 distinct values, so a device-side histogram
 * of the match counts yields that quantile exactly and only the surviving
 * upper-triangle entries (i <= j, diagonal = 1.0 included; zero weights are no
 * edges) leave the GPU, as a (i, j, weight) list sorted by (i, j), 0-based.
 * Call with ei = ej = ew = NULL to obtain threshold and edge count first. */
int da_similarity_mh_edges(const uint8_t *residues, const int64_t *offsets, int64_t n,
                           int k, int n_hash, const uint32_t *seeds, double thresh_p,
                           double *threshold_out, int64_t *n_edges_out,
                           int64_t capacity, int32_t *ei, int32_t *ej, double *ew);
/* The same for similarityNW: matches / length takes few distinct values too (the uint16 code
 * matches << 8 | length), so threshold and edge list come from a histogram of the codes.
 * Sequences up to 127 residues; an empty sequence is refused (its similarities are NaN and
 * R's quantile() stops on NaN).  Errors of da_similarity_nw apply unchanged. */
int da_similarity_nw_edges(const uint8_t *residues, const int64_t *offsets, int64_t n,
                           const char *matrix_name, int gap_open, int gap_ext, double thresh_p,
                           double *threshold_out, int64_t *n_edges_out,
                           int64_t capacity, int32_t *ei, int32_t *ej, double *ew);
/* One-pass form of the two functions above: *_begin runs the pipeline ONCE and parks the sorted edge list in a
 * handle; the caller sizes its vectors from n_edges_out, copies with da_edges_fetch and releases the handle with
 * da_edges_free (the size-query-then-fill convention above runs the whole pipeline twice).  The handle is the one
 * library-owned object of this ABI; it holds host memory only. */
typedef struct da_edges da_edges;
int da_similarity_mh_edges_begin(const uint8_t *residues, const int64_t *offsets, int64_t n,
                                 int k, int n_hash, const uint32_t *seeds, double thresh_p,
                                 da_edges **handle_out, double *threshold_out, int64_t *n_edges_out);
int da_similarity_nw_edges_begin(const uint8_t *residues, const int64_t *offsets, int64_t n,
                                 const char *matrix_name, int gap_open, int gap_ext, double thresh_p,
                                 da_edges **handle_out, double *threshold_out, int64_t *n_edges_out);
/* ... and of the exact Jaccard index (see "the EXACT Jaccard index" above) */
int da_similarity_jaccard_edges(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, double thresh_p, double *threshold_out,
                                int64_t *n_edges_out, int64_t capacity, int32_t *ei, int32_t *ej, double *ew);
int da_similarity_jaccard_edges_begin(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, double thresh_p, da_edges **handle_out,
                                      double *threshold_out, int64_t *n_edges_out);
int da_edges_fetch(const da_edges *handle, int64_t capacity, int32_t *ei, int32_t *ej, double *ew);
void da_edges_free(da_edges *handle);
/* R's quantile(x, p, type = 7) of the multiset {values[b] repeated hist[b] times},
 * values ascending (host arithmetic, no device needed). */
int da_quantile_type7(const uint64_t *hist, const double *values, int nbins, double p, double *q_out);
/* device pieces: histogram of the strict upper triangle of an n x n uint16 matrix
 * (caller zeroes d_hist[nbins]); append of entries flagged in d_keep[nbins]
 * (caller zeroes *d_count; entries beyond `capacity` are counted, not stored).  Both ADD to what they find: a second call
 * into the same d_hist doubles the counts, a second extraction without zeroing *d_count appends.  Only the strict upper
 * triangle is read (with include_diagonal != 0 the diagonal too), through any ld >= n and any 2-byte aligned base.  Keys
 * >= nbins are neither counted nor kept, and the key 65535 is reserved ("not an element"): nbins = 65536 fails with
 * DA_ERR_UNSUPPORTED ("... value 65535 is reserved") before anything is launched -- d_hist, *d_count and the outputs stay
 * as they were.  The same holds for the *_rows and shard forms. */
int da_dev_upper_histogram(const uint16_t *d_compact, int64_t ld, int64_t n, int nbins,
                           uint64_t *d_hist, void *stream);
int da_dev_extract_edges(const uint16_t *d_compact, int64_t ld, int64_t n, const uint8_t *d_keep,
                         int nbins, int include_diagonal, int32_t *d_i, int32_t *d_j, uint16_t *d_v,
                         int64_t capacity, uint64_t *d_count, void *stream);

/* The same two steps on one rank's folded shard block (da_dev_mh_compare_shard output).  Every
 * unordered pair lives on exactly one rank: all-reduce the n_hash+1 histogram words, derive the
 * threshold, and each rank extracts its own (disjoint) edges -- no N x N exchange. */
int da_dev_shard_histogram(const uint16_t *d_local, int64_t ld, int64_t n, int rank, int world,
                           int nbins, uint64_t *d_hist, void *stream);
int da_dev_shard_extract_edges(const uint16_t *d_local, int64_t ld, int64_t n, int rank, int world,
                               const uint8_t *d_keep, int nbins, int include_diagonal,
                               int32_t *d_i, int32_t *d_j, uint16_t *d_v, int64_t capacity,
                               uint64_t *d_count, void *stream);

/* ---- two sets, threshold form: the entries of the m x n rectangle that pass a threshold, as a sorted edge list ----
 * R is the matrix da_similarity_mh_cross / da_similarity_nw_cross return (no forced diagonal).  The result is every (i, j) with
 * R[i][j] >= threshold and R[i][j] > 0 (clusterbreak's pep.sim[pep.sim < threshold] <- 0; a zero weight is no edge), sorted by (i, j),
 * 0-based, weight bit for bit R[i][j]; the m x n matrix never exists.
 *   thresh_is_quantile == 0: threshold = thresh, any non-NaN double (a range query: "every y within t of each x");
 *   thresh_is_quantile != 0: threshold = quantile(as.vector(R), thresh), R's type 7 over all m * n entries, 0 <= thresh <= 1 -- from a
 *                            device histogram of the uint16 counts / codes and da_quantile_type7 (NW: on the codes in ascending order of
 *                            their value, as da_similarity_nw_edges).
 * The decision is made on the host per count / code and uploaded as a byte table -- MinHash keep[c] = c > 0 && (double)c / (double)n_hash
 * >= threshold, NW keep[code] = matches > 0 && (double)matches / (double)length >= threshold -- with the library's own divide, so the
 * boundary R == threshold is exact.  *_begin fills a da_edges handle: read it with da_edges_fetch, release it with da_edges_free.
 * Validation, before any device is needed: everything da_similarity_*_cross checks, in its order and with its texts; then the threshold
 * argument (quantile form: thresh outside [0, 1] or NaN; absolute form: NaN -> DA_ERR_BAD_ARG); then, for NW, the limits of
 * da_similarity_nw_cross_topk: every sequence on both sides has 1 .. 127 residues (DA_ERR_UNSUPPORTED; a NaN has no place in a quantile).
 * NW with m == 0 or n == 0: DA_OK and no edges in the absolute form, DA_ERR_BAD_ARG "quantile of an empty set" in the quantile form.
 * The rectangle is computed as uint16 codes in row blocks of x (operand, padding, 131 068-row rule and DYNAALIGN_BLOCK_BYTES blocking of
 * da_similarity_*_cross_topk).  Absolute form: ONE pass -- per block the compare, the per-row counts, the 8-byte total read back, the
 * edge buffers sized from it, the ordered emit.  Quantile form: a first pass of compare + histogram per block, the threshold on the
 * host, then the pass above; a rectangle that fits ONE block is kept from the first pass, one cut into several blocks is compared
 * twice.  Single device, the direct route only. */
int da_similarity_mh_cross_edges_begin(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m,
                                       const uint8_t *y_residues, const int64_t *y_offsets, int64_t n,
                                       int k, int n_hash, const uint32_t *seeds, double thresh, int thresh_is_quantile,
                                       da_edges **handle_out, double *threshold_out, int64_t *n_edges_out);
int da_similarity_nw_cross_edges_begin(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m,
                                       const uint8_t *y_residues, const int64_t *y_offsets, int64_t n,
                                       const char *matrix_name, int gap_open, int gap_ext, double thresh, int thresh_is_quantile,
                                       da_edges **handle_out, double *threshold_out, int64_t *n_edges_out);

/* The device pieces, on a block of uint16 keys: `rows` rows of ld >= n keys.  Rows are read in 16-byte units where their address allows
 * it, in 2-byte units otherwise: every ld and base address works.  All are asynchronous on `stream`.  NULL pointers, ld < n and nbins
 * outside 1 .. 65536 are DA_ERR_BAD_ARG; rows == 0 is DA_OK and touches nothing.
 * da_dev_rect_histogram: d_hist[v] += the number of keys equal to v in the whole block (the caller zeroes d_hist[nbins]); keys >= nbins are
 *   ignored.  Persistent workgroups with an LDS histogram for nbins <= 8192, global atomics beyond; key 0 is counted in a register.
 * da_dev_threshold_rows_count: d_rowptr[r] = the number of keys v < nbins with d_keep[v] != 0 in the rows before r (an exclusive scan of
 *   the per-row counts): the first slot of row r, and d_rowptr[rows] the block's total (int64, rows + 1 entries).  d_work:
 *   da_dev_threshold_rows_workspace_bytes(rows) bytes.
 * da_dev_threshold_rows_emit: for every row its kept columns in ASCENDING column order at d_j[d_rowptr[r] ...] (int32) with their keys
 *   in d_key_out (uint16); slots >= capacity are not written (d_rowptr already says how many there are).  d_keep and the keys must be those
 *   the count saw.  An ordered compaction -- a workgroup per row (one wave for rows of up to 1024 keys) walks it in chunks of 8 keys per
 *   thread, scans the per-thread kept counts and carries a running base -- with no output atomic and no sort. */
int da_dev_rect_histogram(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, int nbins, uint64_t *d_hist, void *stream);
size_t da_dev_threshold_rows_workspace_bytes(int64_t rows);
int da_dev_threshold_rows_count(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, const uint8_t *d_keep, int nbins,
                                int64_t *d_rowptr, void *d_work, size_t work_bytes, void *stream);
int da_dev_threshold_rows_emit(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, const uint8_t *d_keep, int nbins,
                               const int64_t *d_rowptr, int32_t *d_j, uint16_t *d_key_out, int64_t capacity, void *stream);

/* The threshold form of similarityMH_cross on two resident sets as ONE call; the result is CSR over the rows of x: d_rowptr[m + 1]
 * (int64), d_j (int32 columns, ascending within a row) and d_w (float64, bit for bit R: (double)count / (double)n_hash) with room for
 * `capacity` entries (d_j / d_w may be NULL when capacity is 0).  *threshold_out and *n_edges_out are HOST values.  If *n_edges_out >
 * capacity the row pointers are complete, the first `capacity` slots are filled and the call returns DA_OK: call again with larger
 * buffers.  Operand and row blocks as da_dev_similarity_mh_cross_topk; the quantile form makes two passes (see above).  Direct route only;
 * n_hash <= 65535; one stream, which it synchronises.  Validates like da_dev_similarity_mh_cross_topk, before it looks at a pointer. */
int da_dev_similarity_mh_cross_edges(const uint8_t *d_x_residues, const int64_t *d_x_offsets, int64_t m,
                                     const uint8_t *d_y_residues, const int64_t *d_y_offsets, int64_t n,
                                     int k, int n_hash, const uint32_t *d_seeds, double thresh, int thresh_is_quantile,
                                     int64_t *d_rowptr, int32_t *d_j, double *d_w, int64_t capacity,
                                     double *threshold_out, int64_t *n_edges_out, void *stream);

/* ---- the NW threshold forms for sequences of up to 1024 residues: 32-bit value ranks in place of the uint16 code ----
 * da_similarity_nw_edges_long_begin has the contract of da_similarity_nw_edges_begin word for word -- arguments, the da_edges handle, the
 * validation order and its texts (matrix name, NULL, n < 2, thresh_p, offsets, residues, an empty sequence, DA_ERR_NO_DEVICE last), the result:
 * threshold = R's type-7 quantile of the strict upper triangle of similarityNW(x), the edges every (i, j), i <= j, diagonal included, with
 * R >= threshold and R > 0, sorted by (i, j), weights bit for bit -- with ONE change: the length refusal (DA_ERR_UNSUPPORTED) is for a
 * sequence of more than 1024 residues.  da_similarity_nw_cross_edges_long_begin is da_similarity_nw_cross_edges_begin in the same way (both
 * forms, the empty-rectangle rules, x[i] is sequence1): 1 .. 1024 residues on both sides.
 * The DP writes DA_OUT_PACK32 codes (matches << 16 | length) in row blocks -- rows [b0, b1) against columns [b0, n) of the square problem,
 * or against the columns of y -- of DYNAALIGN_BLOCK_BYTES at 4 bytes per element (half the free device memory without it; a multiple of 8
 * rows, at least 8); a square problem
 * that fits one block runs the symmetric sweep, every pair once.  Each code is replaced by the dense rank of its double value
 * (da_nw_value_ranks: equal values from different codes, 128/256 and 150/300, are ONE rank), and histogram, keep decision and emitted key
 * work on ranks: threshold = da_quantile_type7(histogram, values); kept = rank >= max(r_thr, 1), r_thr the smallest rank whose value is >=
 * threshold, so the boundary R == threshold is exact; weight = values[rank].  Quantile form: a problem that fits one block stays resident
 * between the histogram and the emit pass, one cut into several blocks runs the DP twice; the absolute form makes one pass.  No
 * duplicate route, single device.  (Top-k on the same ranks: da_similarity_nw_knn_long, below.) */
int da_similarity_nw_edges_long_begin(const uint8_t *residues, const int64_t *offsets, int64_t n,
                                      const char *matrix_name, int gap_open, int gap_ext, double thresh_p,
                                      da_edges **handle_out, double *threshold_out, int64_t *n_edges_out);
int da_similarity_nw_cross_edges_long_begin(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m,
                                            const uint8_t *y_residues, const int64_t *y_offsets, int64_t n,
                                            const char *matrix_name, int gap_open, int gap_ext, double thresh, int thresh_is_quantile,
                                            da_edges **handle_out, double *threshold_out, int64_t *n_edges_out);

/* The value table of the NW codes of sequences up to max_len (1 .. 1024) residues.  Over 1 <= length <= 2 * max_len, 0 <= matches <=
 * min(length, max_len): values_out[D] = the distinct doubles (double)matches / (double)length, ascending (values_out[0] = 0.0), and
 * rank_out[length * (max_len + 1) + matches] (uint32, (2 * max_len + 1) * (max_len + 1) entries) = the dense rank of that double: equal
 * doubles get equal ranks, a larger double a larger rank, rank 0 <=> matches == 0.  Entries outside that set (length 0, matches > length)
 * are 0.  *n_values_out = D (1 301 496 at 1024).  values_out == rank_out == NULL: size query.  Host only; needs no device. */
int da_nw_value_ranks(int max_len, double *values_out, int64_t *n_values_out, uint32_t *rank_out);

/* The device pieces, on a block of uint32 keys: `rows` rows of ld >= n keys, read in 16-byte units where a row's address allows it and in
 * 4-byte units otherwise: every ld and 4-byte-aligned base works.  All are asynchronous on `stream`.  NULL pointers, ld < n, nbins outside
 * 1 .. 2^31 - 1 and a negative row_begin / col_begin are DA_ERR_BAD_ARG; rows == 0 is DA_OK and touches nothing.
 * triangle != 0: the block is rows [row_begin, row_begin + rows) x columns [col_begin, col_begin + n) of a square problem and an element's
 *   global position decides whether it is looked at; triangle == 0: the whole rectangle (row_begin / col_begin unused).
 * da_dev_nw_codes_to_ranks: d_out[r][c] = d_rank[length * (max_len + 1) + matches] of the PACK32 code d_codes[r][c] (d_rank: the table of
 *   da_nw_value_ranks(max_len) on the device); a code outside the table's domain (length 0, length > 2 * max_len, matches > max_len, matches
 *   > length) gets rank 0 and reads nothing.  d_out == d_codes (with ld_out == ld) is allowed.
 * da_dev_rank_histogram: d_hist[v] += the number of keys equal to v (the caller zeroes uint64 d_hist[nbins]); keys >= nbins are ignored.
 *   triangle: only elements with global column > global row (the strict upper triangle) are counted.  Equal keys are merged before any
 *   atomic -- within a wave (one lane adds the count of all lanes holding its key), then in a 4096-slot LDS cache per workgroup that is
 *   flushed once -- so a block that is mostly one key does not serialise on its bin.
 * da_dev_threshold_ranks_count: d_rowptr[r] = the number of kept elements in the rows before r (int64, rows + 1 entries; d_rowptr[rows] is
 *   the block's total); kept: r_min <= key < nbins, and with triangle global column >= global row (the diagonal INCLUDED).  d_work:
 *   da_dev_threshold_rows_workspace_bytes(rows) bytes.
 * da_dev_threshold_ranks_emit: for every row its kept columns -- LOCAL to the block, 0 .. n - 1 -- in ASCENDING order at
 *   d_j[d_rowptr[r] ...] (int32) with their keys in d_key_out (uint32); slots >= capacity are not written.  Same arguments as the count.
 *   A workgroup per row (one wave for rows of up to 1024 keys), 4 keys per thread per chunk, no output atomic and no sort; a row without
 *   an edge is not read again, and the part of a row left of the diagonal is not read at all. */
int da_dev_nw_codes_to_ranks(const uint32_t *d_codes, int64_t rows, int64_t n, int64_t ld, int max_len, const uint32_t *d_rank,
                             uint32_t *d_out, int64_t ld_out, void *stream);
int da_dev_rank_histogram(const uint32_t *d_keys, int64_t rows, int64_t n, int64_t ld, int64_t nbins, uint64_t *d_hist, int triangle,
                          int64_t row_begin, int64_t col_begin, void *stream);
int da_dev_threshold_ranks_count(const uint32_t *d_keys, int64_t rows, int64_t n, int64_t ld, uint32_t r_min, int64_t nbins, int triangle,
                                 int64_t row_begin, int64_t col_begin, int64_t *d_rowptr, void *d_work, size_t work_bytes, void *stream);
int da_dev_threshold_ranks_emit(const uint32_t *d_keys, int64_t rows, int64_t n, int64_t ld, uint32_t r_min, int64_t nbins, int triangle,
                                int64_t row_begin, int64_t col_begin, const int64_t *d_rowptr, int32_t *d_j, uint32_t *d_key_out,
                                int64_t capacity, void *stream);

/* ---- nearest-neighbour lists and top-k for sequences of up to 1024 residues, on 32-bit value ranks ----
 * da_dev_topk_ranks: exact top-k per row of a block of uint32 keys that ARE value ranks (what da_dev_nw_codes_to_ranks leaves): `rows` rows
 * of ld >= n keys, every ld and every 4-byte-aligned base.  Row r of d_idx (int32) / d_key_out (uint32), ld_out >= top elements a row, lists
 * the `top` columns of row r by (rank descending, column ascending) -- numpy's argsort(-row, kind = "stable")[:top] -- and the ranks found
 * there.  nbins (1 .. 2^31 - 1) only places the digits of the radix select: ceil(bits of (nbins - 1) / 8) 8-bit digits, most significant
 * first.  Keys must be < nbins; a key beyond the digits is taken as the largest value they hold: a wrong selection, never an access out of
 * bounds.  The key block is only read.  1 <= top <= n (DA_ERR_BAD_ARG), top <= 1024 (DA_ERR_UNSUPPORTED, da_dev_topk_rows' sentence); NULL
 * pointers, ld < n, ld_out < top, a negative shape and nbins outside its range are DA_ERR_BAD_ARG; rows == 0 is DA_OK and touches nothing.
 * One workgroup per row (one wave for n <= 1024), the row read once per digit and once more (k_topk_ranks).  Asynchronous on `stream`.
 * da_dev_topk_ranks_self: the block is rows [self_col0, self_col0 + rows) of a square problem and row r's own column self_col0 + r is absent
 * from its selection; d_self_key[r] (may be NULL) receives the rank found there, and is left untouched where the own column is outside
 * [0, n).  1 <= top <= n - 1.  Everything else as above (da_dev_topk_rows_self on 32-bit ranks). */
int da_dev_topk_ranks(const uint32_t *d_keys, int64_t rows, int64_t n, int64_t ld, int64_t nbins, int top,
                      int32_t *d_idx, uint32_t *d_key_out, int64_t ld_out, void *stream);
int da_dev_topk_ranks_self(const uint32_t *d_keys, int64_t rows, int64_t n, int64_t ld, int64_t nbins, int top, int64_t self_col0,
                           int32_t *d_idx, uint32_t *d_key_out, int64_t ld_out, uint32_t *d_self_key, void *stream);

/* da_similarity_nw_knn and da_similarity_nw_cross_topk for sequences of 1 .. 1024 residues: the same arguments, the same results (idx, val
 * and diag bit for bit where both apply), the same validation in the same order and with the same texts, DA_ERR_NO_DEVICE last; the one
 * difference is the length refusal, DA_ERR_UNSUPPORTED for a sequence of more than 1024 residues.  `top` is not clamped; val_out / diag_out
 * may be NULL.  Route: upload and encode once; per row block of DYNAALIGN_BLOCK_BYTES (4 bytes a key, a multiple of 8 rows, at least 8) the
 * DP as PACK32 codes, the value ranks in place (da_nw_value_ranks of the call's longest sequence: 128/256 and 150/300 are ONE rank),
 * da_dev_topk_ranks[_self] into [rows][top] index and rank buffers; val = values[rank] and diag = values[own rank] on the host, the
 * library's divide bit for bit.  Only the lists leave the device.  The one-set form needs FULL rows of the square: a square that fits one
 * block runs the symmetric sweep (every pair once, mirrored, the diagonal included); one cut into blocks runs rows [b0, b1) x columns
 * [0, n) with self_col0 = b0 and so computes EVERY PAIR TWICE, once in each of its two rows' blocks -- the price of leaving with the lists
 * only.  Single device; no duplicate route; no device-pointer form. */
int da_similarity_nw_knn_long(const uint8_t *residues, const int64_t *offsets, int64_t n, const char *matrix_name, int gap_open, int gap_ext,
                              int top, int32_t *idx_out, double *val_out, double *diag_out);
int da_similarity_nw_cross_topk_long(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m,
                                     const uint8_t *y_residues, const int64_t *y_offsets, int64_t n,
                                     const char *matrix_name, int gap_open, int gap_ext, int top, int32_t *idx_out, double *val_out);

/* ---- summary statistics of a similarity matrix that never leaves the device (reference R/similarity.R:11-34, compute_similarity_stats) ----
 * S is the n x n matrix da_similarity_mh / da_similarity_nw return for the same arguments, U the P = n (n - 1) / 2 values of its strict
 * upper triangle.
 *   min_similarity, max_similarity   min(U), max(U), bit for bit.
 *   median_similarity                with u = sort(U): u[(P - 1) / 2] for odd P, (u[P / 2 - 1] + u[P / 2]) / 2 in double arithmetic for even P
 *                                    (R's median(); numpy's np.median).  NOT da_quantile_type7(0.5), whose (1 - h) lo + h hi can differ in
 *                                    the last bit.
 *   mean_similarity                  sum over the occupied values, ascending, of count * value, accumulated in long double, divided by P
 *                                    and rounded to double: within 2^-42 relative of the exact mean of the doubles.  R's mean() is a two-pass
 *                                    long double sum over the elements; the two are not bit-identical.
 *   most_similar_pair                R's which(S == max(U), arr.ind = TRUE)[1, ] as 0-based (row, col): the first position in COLUMN-MAJOR
 *                                    order over the WHOLE matrix -- diagonal and lower triangle included -- where S equals max(U); equality
 *                                    is of values (NW's 1/2 and 2/4 are equal).  When a MinHash set holds two sequences with identical
 *                                    signatures, max(U) = 1.0 = S[0][0] and the answer is (0, 0): the reference's behaviour.
 *   least_similar_pair               the same with min(U).
 *   most_similar_upper,              not in the reference: the first (i, j), i < j, in ROW-MAJOR order where S[i][j] equals max(U) / min(U)
 *   least_similar_upper              -- the real pair where the reference's rule lands on the diagonal.
 * The diagonal: MinHash 1.0 (src/minHash.cpp:161); NW whatever the DP gives for (i, i), read from the matrix. */
typedef struct da_similarity_stats {
  double mean_similarity, median_similarity, min_similarity, max_similarity;
  int64_t pairs;                       /* P */
  int64_t most_similar_pair[2], least_similar_pair[2];     /* (row, col), 0-based */
  int64_t most_similar_upper[2], least_similar_upper[2];
} da_similarity_stats;

/* The four numbers from a histogram: the multiset {values[b] repeated hist[b] times}, values ascending; hist must not be all zero.  Any
 * output pointer may be NULL.  Host arithmetic as defined above; needs no device. */
int da_stats_from_histogram(const uint64_t *hist, const double *values, int64_t nbins, double *mean_out, double *median_out,
                            double *min_out, double *max_out);

/* The statistics of similarityMH / similarityNW without the matrix on the host: the compare (or the DP) writes uint16 counts / codes that
 * stay on the device, the histogram of the strict upper triangle gives the four numbers (NW: bins of equal value are merged first), and
 * one more pass (da_dev_upper_extrema) gives every row's extremes with their first columns, 20 bytes a row, from which the host takes the
 * positions.  Validation, before any device is needed, in the order of da_similarity_mh_edges / da_similarity_nw_edges:
 *   MinHash: the reference's three checks, NULL pointers, n < 2, n_hash > 65535 (DA_ERR_UNSUPPORTED), the offsets;
 *   NW: the matrix name, NULL pointers, n < 2, the offsets, the residues (the reference's first-raised message), an empty sequence
 *       (DA_ERR_UNSUPPORTED: its similarities are NaN and R's median() gives NA), a sequence of more than 127 residues -- 1024 for
 *       da_similarity_nw_stats_long (DA_ERR_UNSUPPORTED);
 * DA_ERR_NO_DEVICE comes last.  da_similarity_nw_stats takes the duplicate collapse and the prefix sharing of da_similarity_nw.
 * da_similarity_nw_stats_long works on 32-bit value ranks (da_nw_value_ranks) in row blocks of DYNAALIGN_BLOCK_BYTES like
 * da_similarity_nw_edges_long_begin, with ONE pass of the DP whatever the number of blocks; a square that fits one block runs the
 * symmetric sweep.  Single device; no duplicate route for MinHash (the direct compare). */
int da_similarity_mh_stats(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, int n_hash, const uint32_t *seeds,
                           da_similarity_stats *out);
int da_similarity_nw_stats(const uint8_t *residues, const int64_t *offsets, int64_t n, const char *matrix_name, int gap_open, int gap_ext,
                           da_similarity_stats *out);
int da_similarity_nw_stats_long(const uint8_t *residues, const int64_t *offsets, int64_t n, const char *matrix_name, int gap_open,
                                int gap_ext, da_similarity_stats *out);

/* ---- the exact Jaccard index for sequences of up to 1024 shingle positions (jaccard_long_kernels.hip) ----
 * Each call is the _long sibling of the da_similarity_jaccard* call of its name: the same arguments, results and errors, with the limit
 * len - k + 1 <= 1024 (its text is the short call's with 1024 in place of 127) -- the short calls keep their limit of 127.  The code of a
 * pair is DA_OUT_PACK32, intersection << 16 | union (1 << 16 | 1 for two empty sets); with S the call's largest shingle count (at least
 * 1) every code lies in the domain of da_nw_value_ranks(S) -- 1 <= union <= 2 S, intersection <= min(union, S) -- and wherever an order is
 * needed the calls run the long NW paths on those value ranks: histogram, exact type-7 quantile, ordered count / emit, top-k, extrema.
 *   da_similarity_jaccard_long, _cross_long     doubles from the device, in row blocks of DYNAALIGN_BLOCK_BYTES; a square that fits one
 *                                               block is computed by the symmetric form (every pair once).
 *   da_similarity_jaccard_cross_topk_long, _knn_long   as da_similarity_nw_cross_topk_long / _knn_long, in row blocks; the one-set call
 *                                               computes a block that is the whole square by the symmetric form, else full rows.
 *   da_similarity_jaccard_edges_long_begin      as da_similarity_jaccard_edges_begin (one pass: da_edges_fetch / da_edges_free).
 *   da_similarity_jaccard_cross_edges_long_begin  the two-set threshold form, which the short family lacks (it serves short sequences too):
 *                                               the entries of the m x n matrix with J >= threshold and J > 0, sorted by (i, j); thresh and
 *                                               thresh_is_quantile as da_similarity_nw_cross_edges_begin.  Validation: k <= 0 -> DA_ERR_BAD_K;
 *                                               m <= 0 or n <= 0: the threshold check, then DA_ERR_BAD_ARG "quantile of an empty set" in the
 *                                               quantile form and no edges in the absolute form; NULL pointers, the offsets of x then y, k > 8,
 *                                               the lengths of x then y; the threshold check; DA_ERR_NO_DEVICE last.
 *   da_similarity_jaccard_stats_long            compute_similarity_stats of the matrix without the matrix, as da_similarity_nw_stats_long (one
 *                                               pass of the rectangle kernel whatever the number of blocks).  Validation: the one-set checks,
 *                                               then n < 2 -> DA_ERR_BAD_ARG.  Empty sets are legal: no sequence is refused for being empty.
 * Single device, the direct route only.
 * The device layer.  da_dev_jaccard_sets_long: as da_dev_jaccard_sets with uint16 counts, max_len - k + 1 <= 1024 and ld_keys in
 * da_jaccard_sets_long_ld(max_len, k) (the largest shingle count rounded up to a multiple of 4, at least 4) .. 1024.  One workgroup per
 * sequence sorts its keys in LDS.  da_dev_jaccard_rect_long: as da_dev_jaccard_rect with kind DA_OUT_PACK32 (uint32 codes, 16-byte stores
 * where the address allows) or DA_OUT_F64; a rectangle whose rows and columns are the same range is computed by the symmetric form. */
int da_similarity_jaccard_long(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, double *out);
int da_similarity_jaccard_cross_long(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m,
                                     const uint8_t *y_residues, const int64_t *y_offsets, int64_t n, int k, double *out, int column_major);
int da_similarity_jaccard_cross_topk_long(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m,
                                          const uint8_t *y_residues, const int64_t *y_offsets, int64_t n, int k, int top, int32_t *idx_out,
                                          double *val_out);
int da_similarity_jaccard_knn_long(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, int top, int32_t *idx_out, double *val_out);
int da_similarity_jaccard_edges_long_begin(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, double thresh_p,
                                           da_edges **handle_out, double *threshold_out, int64_t *n_edges_out);
int da_similarity_jaccard_cross_edges_long_begin(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m,
                                                 const uint8_t *y_residues, const int64_t *y_offsets, int64_t n, int k, double thresh,
                                                 int thresh_is_quantile, da_edges **handle_out, double *threshold_out, int64_t *n_edges_out);
int da_similarity_jaccard_stats_long(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, da_similarity_stats *out);
int64_t da_jaccard_sets_long_ld(int64_t max_len, int k);
int da_dev_jaccard_sets_long(const uint8_t *d_residues, const int64_t *d_offsets, int64_t n, int64_t max_len, int k, void *d_keys,
                             int64_t ld_keys, uint16_t *d_counts, void *stream);
int da_dev_jaccard_rect_long(const void *d_keys, const uint16_t *d_counts, int64_t n, int64_t ld_keys, int k, int64_t row_begin,
                             int64_t row_end, int64_t col_begin, int64_t col_end, int kind, void *d_out, int64_t ld, void *stream);

/* ---- the Levenshtein similarity: plain edit distance, on a bit-parallel kernel (lev_kernels.hip) ----
 * Sequences are byte strings, any byte value, no alphabet check; the empty string is legal.  d(a, b) is the Levenshtein distance -- insert,
 * delete and substitute cost 1 each -- L = max(len(a), len(b)), and lev(a, b) = (double)(L - d) / (double)L, one IEEE divide of the two
 * integers; 1.0 for two empty strings, 0.0 when exactly one is empty (d = L).  Nothing is forced on the diagonal: lev(a, a) is 1.0 by the
 * definition.  The matrix is symmetric; no NaN occurs.  With all strings of length L, "within t edits" is the threshold (L - t) / L.
 * The distance is computed in its bit-vector form (Myers 1999, Hyyro's global variant): a column of the DP is one uint32 (the call's longest
 * sequence <= 32 bytes), one uint64 (<= 64) or two uint64 (<= 127), and a pair costs len(b) steps of some seventeen integer operations.
 * uint16 code (DA_OUT_COMPACT): (L - d) << 8 | L, 0x0101 for two empty strings -- the shape of the NW code, valued by the same divide (a
 * code's low byte is never 0).  Wherever an order is needed (top-k, nearest neighbours, the quantile) equal VALUES tie whatever their codes
 * (10/20 and 5/10): the selection runs on da_nw_code_ranks(127, ...), whose domain holds every (L - d, L) the limit allows.
 * Limit (DA_ERR_UNSUPPORTED, the text names the limit and the sequence's 1-based index): every sequence has at most 127 bytes.
 * Validation, before any device is needed: that of the da_similarity_jaccard* call of the same form without k.  One set: n <= 0 ->
 * DA_ERR_EMPTY_INPUT, NULL pointers, the offsets, the sequence lengths; then what the call adds -- _knn: n < 2, top < 1 or top > n - 1 ->
 * DA_ERR_BAD_ARG, top > 1024 -> DA_ERR_UNSUPPORTED; _edges: n < 2, thresh_p outside [0, 1] -> DA_ERR_BAD_ARG.  Two sets: m <= 0 or n <= 0 returns
 * DA_OK and writes nothing (_cross_topk: m <= 0 returns DA_OK, n <= 0 with m > 0 is DA_ERR_BAD_ARG; _cross_edges_begin: no edges in the absolute
 * form, DA_ERR_BAD_ARG "quantile of an empty set" in the quantile form, after the check of thresh); NULL pointers, the offsets of x then y, the
 * lengths of x then y; then top (the texts of da_similarity_nw_cross_topk) or thresh (those of da_similarity_nw_cross_edges_begin).
 * DA_ERR_NO_DEVICE comes last.
 *   da_similarity_lev              out: n * n doubles (the device writes uint16 codes, the host widens them).
 *   da_similarity_lev_cross        out: m x n, bit for bit the block [0:m, m:m+n] of da_similarity_lev on c(x, y); column_major as
 *                                  da_similarity_mh_cross.  Both sets form ONE operand [x ; y] on the device.
 *   da_similarity_lev_cross_topk   idx_out [m][top] int32, val_out [m][top] float64 or NULL: numpy's argsort(-R, axis = 1, kind = "stable")[:, :top].
 *   da_similarity_lev_knn          idx_out / val_out [n][top]: the `top` columns j != i of every row, as da_similarity_jaccard_knn.
 *   da_similarity_lev_edges[_begin]  threshold = R's type-7 quantile of the strict upper triangle at thresh_p; the edges i <= j, diagonal
 *                                  included, with lev >= threshold and lev > 0, sorted by (i, j); conventions of da_similarity_nw_edges[_begin].
 *   da_similarity_lev_cross_edges_begin  the range query: every (i, j) with R[i, j] >= threshold and R[i, j] > 0, sorted by (i, j); thresh is
 *                                  an absolute threshold, or with thresh_is_quantile != 0 the level of R's type-7 quantile over all m * n entries;
 *                                  conventions of da_similarity_nw_cross_edges_begin (da_edges_fetch / da_edges_free).
 * Single device, the direct route only; top-k / kNN / the range query work in row blocks of DYNAALIGN_BLOCK_BYTES.
 * The device layer.  The bytes that occur in a call are numbered as classes 0 .. n_classes - 1 (1 <= n_classes <= 256) by class_map, a HOST array of
 * 256 class ids, each below n_classes; bytes that do not occur may map to any class.  da_dev_lev_masks writes the operand of da_dev_lev_rect into
 * d_masks (8-byte aligned, masks_bytes >= da_dev_lev_masks_bytes(n, max_len, n_classes); 0 for arguments outside the limits): per sequence and class
 * the match mask -- bit p of the mask of class c is set iff byte p has class c -- the class ids of its bytes, and its length.  max_len: the longest
 * sequence (<= 127); it chooses the word shape, so both calls must be given the same n, max_len and n_classes.  n <= 0 -> DA_ERR_EMPTY_INPUT, NULL
 * pointers -> DA_ERR_BAD_ARG, max_len > 127 -> DA_ERR_UNSUPPORTED, n_classes or a class id out of range, d_masks misaligned or too small -> DA_ERR_BAD_ARG.
 * da_dev_lev_rect: rows [row_begin, row_end) x columns [col_begin, col_end) of the n sequences, element (i, j) = lev(sequence i, sequence j), as
 * DA_OUT_COMPACT codes or DA_OUT_F64 doubles at d_out[(i - row_begin) * ld + (j - col_begin)]; any ld >= columns and any naturally aligned d_out
 * (16-byte stores where the address allows, single elements otherwise); every element written once, nothing else touched; an empty rectangle is
 * DA_OK.  A rectangle whose rows and columns are the same range is computed by the symmetric form.  Two sets are compared through the operand of
 * their concatenation.  Both calls are asynchronous on `stream`. */
int da_similarity_lev(const uint8_t *residues, const int64_t *offsets, int64_t n, double *out);
int da_similarity_lev_cross(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m,
                            const uint8_t *y_residues, const int64_t *y_offsets, int64_t n, double *out, int column_major);
int da_similarity_lev_cross_topk(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m,
                                 const uint8_t *y_residues, const int64_t *y_offsets, int64_t n, int top, int32_t *idx_out, double *val_out);
int da_similarity_lev_knn(const uint8_t *residues, const int64_t *offsets, int64_t n, int top, int32_t *idx_out, double *val_out);
int da_similarity_lev_edges(const uint8_t *residues, const int64_t *offsets, int64_t n, double thresh_p, double *threshold_out,
                            int64_t *n_edges_out, int64_t capacity, int32_t *ei, int32_t *ej, double *ew);
int da_similarity_lev_edges_begin(const uint8_t *residues, const int64_t *offsets, int64_t n, double thresh_p, da_edges **handle_out,
                                  double *threshold_out, int64_t *n_edges_out);
int da_similarity_lev_cross_edges_begin(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m,
                                        const uint8_t *y_residues, const int64_t *y_offsets, int64_t n, double thresh, int thresh_is_quantile,
                                        da_edges **handle_out, double *threshold_out, int64_t *n_edges_out);
size_t da_dev_lev_masks_bytes(int64_t n, int64_t max_len, int n_classes);
int da_dev_lev_masks(const uint8_t *d_residues, const int64_t *d_offsets, int64_t n, int64_t max_len, const uint8_t *class_map, int n_classes,
                     void *d_masks, size_t masks_bytes, void *stream);
int da_dev_lev_rect(const void *d_masks, int64_t n, int64_t max_len, int n_classes, int64_t row_begin, int64_t row_end, int64_t col_begin,
                    int64_t col_end, int kind, void *d_out, int64_t ld, void *stream);

/* The device piece.  The block: `rows` rows of ld >= n keys, rows [row_begin, row_begin + rows) x columns [col_begin, col_begin + n) of a
 * square problem (the origin convention of da_dev_rank_histogram).  d_records[r], for the elements of row r whose global column is
 * greater than the global row: the smallest and the largest rank and the smallest block-local column holding each; a row without such an
 * element has min_col = max_col = -1 (min_key = 0xFFFFFFFF, max_key = 0).  diag_key is the rank of the element at global column ==
 * global row, 0xFFFFFFFF when it lies outside the block.
 *   da_dev_upper_extrema: uint16 keys; rank = d_rank[key] with d_rank the 65 536-entry table of da_nw_code_ranks on the device (as
 *     da_dev_topk_rows uses it), or the key itself when d_rank is NULL (MinHash counts).
 *   da_dev_upper_extrema32: uint32 keys that are value ranks already (da_dev_nw_codes_to_ranks).
 * A workgroup per row (one wave when no row has more than 1024 such elements); 16-byte loads where a row's address allows it, single keys
 * otherwise: every ld and naturally aligned base works.  What lies left of the diagonal is not read in whole chunks, apart from the
 * diagonal element.  No atomics.  Asynchronous on `stream`; NULL pointers, ld < n, a negative shape or origin are DA_ERR_BAD_ARG;
 * rows == 0 is DA_OK and touches nothing. */
typedef struct da_row_extrema {
  uint32_t min_key;
  int32_t min_col;
  uint32_t max_key;
  int32_t max_col;
  uint32_t diag_key;
} da_row_extrema;
int da_dev_upper_extrema(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, const uint16_t *d_rank, int64_t row_begin,
                         int64_t col_begin, da_row_extrema *d_records, void *stream);
int da_dev_upper_extrema32(const uint32_t *d_keys, int64_t rows, int64_t n, int64_t ld, int64_t row_begin, int64_t col_begin,
                           da_row_extrema *d_records, void *stream);

/* ---- the caller's clustering step (reference R/clusterbreak.R:112-136, netcluster) ------------
 * igraph::cluster_louvain(graph_from_adjacency_matrix(S, mode = "upper", weighted = TRUE),
 *                         weights = E(g)$weight, resolution = 1.05)$membership
 * on an edge list (i, j, weight), 0-based, i == j = self-loop (the thresholded matrix keeps its 1.0
 * diagonal, R/clusterbreak.R:221), (i, j) and (j, i) the same undirected edge.  HOST code, like igraph in
 * the reference: multilevel modularity optimisation with igraph's conventions (loops count twice in a
 * vertex's strength; the last level's membership, renumbered 1.. by first appearance).  Deterministic in
 * (graph, seed) whatever the order of the edge arrays; igraph's own result depends on R's RNG stream and
 * is not reproducible outside R.  membership_out: n_vertices ids starting at 1; modularity_out /
 * levels_out may be NULL. */
int da_louvain(int64_t n_vertices, int64_t n_edges, const int32_t *ei, const int32_t *ej, const double *ew,
               double resolution, uint32_t seed, int32_t *membership_out, double *modularity_out,
               int32_t *levels_out);
/* The same clustering from a graph that is already canonical: symmetric CSR (both directions of every edge, columns ascending and
 * distinct, no diagonal entries), weights as codes into values[n_values], self-loops per vertex as codes (0xFFFF = none; NULL = none).
 * Identical result to da_louvain on the corresponding edge list.  da_dev_edges_to_csr builds exactly this on the device from the
 * (i <= j, code) list of da_dev_extract_edges[_rows]: d_work = da_dev_edges_to_csr_bytes(n_edges, n) bytes (256-byte aligned),
 * d_ptr[n + 1], d_adj / d_codes with room for 2 n_edges entries, d_loops[n]; d_ptr[n] = number of entries written. */
int da_louvain_csr(int64_t n_vertices, const int64_t *ptr, const int32_t *adj, const uint16_t *codes, const uint16_t *loop_codes,
                   const double *values, int32_t n_values, double resolution, uint32_t seed, int32_t *membership_out,
                   double *modularity_out, int32_t *levels_out);
size_t da_dev_edges_to_csr_bytes(int64_t n_edges, int64_t n);
int da_dev_edges_to_csr(const int32_t *d_i, const int32_t *d_j, const uint16_t *d_v, int64_t n_edges, int64_t n, void *d_work,
                        size_t work_bytes, int64_t *d_ptr, int32_t *d_adj, uint16_t *d_codes, uint16_t *d_loops, void *stream);

/* The synchronous Louvain on that CSR where it lies, in device memory: the clustering function clusterbreak.louvain_sync_dense defines in
 * numpy, reproduced bit for bit (membership, modularity, levels, iterations).  It is NOT da_louvain: another algorithm with other
 * memberships.  Weights become integers rint(w * 2^30), all sums of weights are exact 64-bit integers; a level is at most 64 iterations of
 * 8 sub-rounds (vertex classes ((v * 2654435761 + seed * 40503 + level) >> 7) & 7), each sub-round one decide launch per degree bin and one
 * apply launch; at most 32 levels.  d_ptr / d_adj / d_codes / d_loops: what da_dev_edges_to_csr wrote (d_loops may be NULL: no self-loops);
 * `values` is HOST memory, n_values <= 65535.  k_lv_validate checks, before anything indexes by a neighbour id or a code, that row pointers
 * start at 0 and do not decrease, that neighbours are in range, ascending, distinct and not the row itself, and that codes are below
 * n_values: a violation returns DA_ERR_BAD_ARG and launches nothing further.  Symmetry of the adjacency is NOT checked: an asymmetric
 * input gives an unspecified clustering (no out-of-range access).  Negative or non-finite values are refused; a graph whose total weight
 * (d_ptr[n] + 2 n) * max(values) * 2^30 could reach 2^62, or with 2^31 - 256 or more entries, returns DA_ERR_UNSUPPORTED.
 * d_work: da_dev_louvain_workspace_bytes(n, d_ptr[n]) bytes, 256-byte aligned (about 56 bytes per adjacency entry: the aggregation sorts
 * one 64-bit key per entry that leaves its community).  d_membership: n ids from 1 in order of first appearance (device memory).
 * modularity_out, levels_out and iterations_out[32] (host memory) may be NULL.  n < 0, NULL pointers and a workspace too small for n are
 * refused before the device is touched; n == 0 returns DA_OK.  The call synchronises `stream`.  da_dev_louvain_workspace_bytes (and the
 * workspace check above) asks hipcub for the scratch sizes of its sort, reduce-by-key and scan: size queries that launch nothing and need
 * no device, as in the LSH entries.  n and nnz outside what the call accepts (n > 2^31 - 16, nnz >= 2^31 - 256, negative) are clamped to those
 * limits for the size; the call itself refuses them. */
size_t da_dev_louvain_workspace_bytes(int64_t n, int64_t nnz);
int da_dev_louvain_csr(int64_t n, const int64_t *d_ptr, const int32_t *d_adj, const uint16_t *d_codes, const uint16_t *d_loops,
                       const double *values, int32_t n_values, double resolution, uint32_t seed, void *d_work, size_t work_bytes,
                       int32_t *d_membership, double *modularity_out, int32_t *levels_out, int32_t *iterations_out /* [32] */, void *stream);

/* ---- connected components: single-linkage groups of a graph, n labels and no edge list out ----------------------------------------------
 * The definition every entry below reproduces element for element is clusterbreak.components_dense (numpy): the graph is undirected on
 * the vertices 0 .. n - 1; edges come in any order and either orientation; repeats and self-loops are harmless; a vertex without an edge
 * is its own component.  With min C(v) the smallest vertex of v's component, membership[v] = 1 + the number of component minima below
 * min C(v): ids from 1 in order of first appearance, the convention of every membership here.  The result is a set property of the graph,
 * so it is deterministic: it depends on neither the order of the edges nor the scheduling of the device.
 *
 * da_components: HOST code, a union-find in plain C++; needs no device.  The CPU twin of the device calls and the fallback for small
 *   graphs.  n < 0, n_edges < 0, n > 2^31 - 16, a NULL n_components_out, a NULL membership_out with n > 0 and NULL edge arrays with
 *   n_edges > 0 are refused first (DA_ERR_BAD_ARG); n == 0 returns DA_OK with 0 components; an endpoint outside [0, n) returns
 *   DA_ERR_BAD_ARG naming the edge, before anything is indexed by it. */
int da_components(int64_t n, int64_t n_edges, const int32_t *ei, const int32_t *ej, int32_t *membership_out, int64_t *n_components_out);
/* The device calls, on graphs that lie in device memory.  A lock-free union-find in 32-bit words: the larger of two roots is hooked under
 * the smaller with one compare-and-swap that expects it to be a root still; a failed swap re-finds from the value it read.  At every
 * instant parent[x] <= x, parent[x] is a vertex of x's component, and a vertex that stopped being a root stays one no more -- so a tree's
 * root is the minimum of its vertices and the labels do not depend on scheduling.  No lane waits for another; there is no flag, no lock and
 * no host loop: validate, init, ONE union launch, compress, flag roots, one exclusive sum, label.  find does not shorten paths (DESIGN.md
 * section 7).  k_cc_validate checks, before anything indexes by an endpoint, that every listed endpoint is in [0, n) -- filtered edges
 * included -- and, for the CSR, that the row pointers start at 0, do not decrease and end at nnz = d_ptr[n]: a violation returns
 * DA_ERR_BAD_ARG and launches nothing further.
 * All three: d_membership int32[n] (device); d_sizes may be NULL, else int32[n] (device): entry c - 1 = the size of component c, the entries
 * from n_components on 0; *n_components_out is host memory.  n < 0, n_edges < 0, NULL pointers and a workspace that is too small are refused
 * before the device is touched (DA_ERR_BAD_ARG); n == 0 returns DA_OK with 0 components and reads nothing; n > 2^31 - 16 returns
 * DA_ERR_UNSUPPORTED.  Edge counts are 64-bit.  The calls synchronise `stream` (one total is read back; the validation reads one word).
 * da_dev_components_workspace_bytes: the parent array, the root flags, the scan output and the hipcub scratch, about 12 bytes per vertex; any
 *   alignment.  A size query that launches nothing and needs no device; n outside [0, 2^31 - 16] is clamped for the size.
 * da_dev_components_edges: an edge list d_i / d_j (int32, n_edges entries).  d_code may be NULL; otherwise only the edges with
 *   d_code[e] >= min_code count (uint16 codes, e.g. the counts of da_dev_lsh_edges or the codes of da_dev_extract_edges): one list can be
 *   cut at several thresholds without being recomputed.
 * da_dev_components_csr: the d_ptr (int64[n + 1]) / d_adj (int32[d_ptr[n]]) that da_dev_edges_to_csr and the kNN graphs produce; codes and
 *   loops are not needed.  symmetric != 0 says the CSR holds both directions of every edge: only the entries with adj > row are united,
 *   which halves the work (an asymmetric CSR passed as symmetric loses the edges listed in their lower direction only).  Rows need not
 *   be sorted; diagonal entries and repeats are harmless.  A wave takes a row of up to 64 entries, the workgroup a longer one. */
size_t da_dev_components_workspace_bytes(int64_t n);
int da_dev_components_edges(const int32_t *d_i, const int32_t *d_j, const uint16_t *d_code /* may be NULL */, int min_code, int64_t n_edges,
                            int64_t n, void *d_work, size_t work_bytes, int32_t *d_membership, int32_t *d_sizes /* may be NULL, n entries */,
                            int64_t *n_components_out, void *stream);
int da_dev_components_csr(int64_t n, const int64_t *d_ptr, const int32_t *d_adj, int symmetric, void *d_work, size_t work_bytes,
                          int32_t *d_membership, int32_t *d_sizes, int64_t *n_components_out, void *stream);

/* ---- MinHash LSH banding: the threshold graph of ONE set from bucketed candidates, not from all n (n - 1) / 2 pairs ---------------------
 * sig = the n x n_hash signatures of da_minhash_signatures.  bands >= 1, rows >= 1, bands * rows <= n_hash; band t = columns
 * [t * rows, (t + 1) * rows); columns >= bands * rows belong to no band but count.  cand(i, j): some band agrees in all its columns.
 * c(i, j) = |{h < n_hash : sig[i][h] == sig[j][h]}|.  The edge set, sorted by (i, j), 0-based:
 *     (i, i, 1.0) for every i   and   (i, j, c / n_hash) for i < j with cand(i, j) and (double)c / (double)n_hash >= threshold
 * -- EXACT with respect to this definition (a bucket key is a hash, but a pair is emitted only after the band's columns were compared
 * themselves); approximate is only the definition's relation to the all-pairs threshold graph: a pair above the threshold that agrees in
 * no whole band is missing.  P(cand) = 1 - (1 - s^rows)^bands for a pair of similarity s.
 *
 * da_similarity_mh_lsh_edges_begin: host boundary, result in a da_edges handle (da_edges_fetch / da_edges_free).  Checks, in this order
 * and before any device is needed: n <= 0 (DA_ERR_EMPTY_INPUT), k, n_hash, NULL pointers, offsets, then DA_ERR_BAD_ARG for bands < 1,
 * rows < 1, bands * rows > n_hash, a threshold outside [0, 1] or NaN, max_candidates < 0, then DA_ERR_UNSUPPORTED for n_hash > 65535.
 * n = 1 is valid (the one diagonal edge).  max_candidates caps the (pair, band) incidences -- pairs of members of one bucket, summed over
 * the buckets -- which are known before any pair is compared: more gives DA_ERR_UNSUPPORTED, the message naming the count, the cap and the
 * largest bucket.
 * da_mh_lsh_last_route: what the calling thread's last LSH call (host or da_dev_lsh_edges) did -- buckets, (pair, band) incidences,
 * distinct candidate pairs (each verified in its first agreeing band) and edges (diagonal included).  NULL pointers are skipped. */
int da_similarity_mh_lsh_edges_begin(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, int n_hash, const uint32_t *seeds,
                                     int bands, int rows, double threshold, int64_t max_candidates, da_edges **handle_out,
                                     int64_t *n_edges_out);
int da_mh_lsh_last_route(int64_t *buckets_out, int64_t *incidences_out, int64_t *verified_pairs_out, int64_t *edges_out);
/* The device pieces, on signatures resident in HBM (row i at d_sig + i * ld_sig; columns >= n_hash are never read, and
 * da_dev_lsh_band_keys reads columns < bands * rows only).  Asynchronous on `stream` unless stated.
 * da_dev_lsh_band_keys: element q = i * bands + t  ->  d_keys[q] = t << 48 | 48 bits of a hash of band t's values of row i, d_ids[q] = i.
 *   Equal band values give equal keys; different values give different keys but for hash collisions.
 * da_dev_lsh_verify_pairs: the per-pair decision on LISTED triples (i, j, band), which need not be ones the pipeline would produce:
 *   d_count[p] = c(i, j); d_keep[p] = 1 when `band` agrees in all its columns, no earlier band does, and
 *   (double)c / (double)n_hash >= threshold -- else 0.  A triple with an index outside [0, n) or a band outside [0, bands) gets 0 / 0.
 * da_dev_lsh_edges: the whole pipeline.  d_work: da_dev_lsh_workspace_bytes(n, bands) bytes, any alignment (the per-incidence and
 *   per-edge buffers are sized by the data and allocated inside).  *n_edges_out = the number of edges; the first min(capacity, that)
 *   of them, in (i, j) order, go to d_i / d_j / d_count (count = c, the diagonal's n_hash), which may be NULL when capacity is 0.
 *   Synchronises the stream (two totals are read back).  n * bands must stay below 2^31 - 256. */
size_t da_dev_lsh_workspace_bytes(int64_t n, int bands);
int da_dev_lsh_band_keys(const uint32_t *d_sig, int64_t n, int64_t ld_sig, int n_hash, int bands, int rows, uint64_t *d_keys,
                         int32_t *d_ids, void *stream);
int da_dev_lsh_verify_pairs(const uint32_t *d_sig, int64_t n, int64_t ld_sig, int n_hash, int bands, int rows, double threshold,
                            const int32_t *d_i, const int32_t *d_j, const int32_t *d_band, int64_t n_triples, uint16_t *d_count,
                            uint8_t *d_keep, void *stream);
int da_dev_lsh_edges(const uint32_t *d_sig, int64_t n, int64_t ld_sig, int n_hash, int bands, int rows, double threshold,
                     int64_t max_candidates, void *d_work, size_t work_bytes, int32_t *d_i, int32_t *d_j, uint16_t *d_count,
                     int64_t capacity, int64_t *n_edges_out, void *stream);
/* The connected components of that edge set -- near-duplicate families, single-linkage clusters at the cut -- without the edge list:
 * membership as da_components gives it on the edges of da_dev_lsh_edges for the same arguments (the definition above).  One set only.
 * da_dev_lsh_components: buckets -> the enumerated verify -> the union step on every kept slot (k_lsh_union) -> compress -> renumber.  No
 *   emit, no 64-bit keys, no edge sort.  d_work: da_dev_lsh_workspace_bytes(n, bands) + da_dev_components_workspace_bytes(n) bytes, any
 *   alignment.  d_membership int32[n], d_sizes NULL or int32[n] (device), *n_components_out host.  n == 0 returns DA_OK with 0 components;
 *   otherwise the checks of da_dev_lsh_edges, all before the device is touched.  Synchronises the stream.  da_mh_lsh_last_route reports
 *   buckets, incidences and verified pairs as for the edge form; `edges` = the kept pairs + n, the number the edge form would have
 *   emitted, so the two calls can be compared.
 * da_similarity_mh_lsh_components: host boundary; membership_out int32[n].  Checks everything da_similarity_mh_lsh_edges_begin checks, in
 *   its order and with its texts, before any device is needed; then n_hash > 65535 (DA_ERR_UNSUPPORTED). */
int da_dev_lsh_components(const uint32_t *d_sig, int64_t n, int64_t ld_sig, int n_hash, int bands, int rows, double threshold,
                          int64_t max_candidates, void *d_work, size_t work_bytes, int32_t *d_membership, int32_t *d_sizes,
                          int64_t *n_components_out, void *stream);
int da_similarity_mh_lsh_components(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, int n_hash, const uint32_t *seeds,
                                    int bands, int rows, double threshold, int64_t max_candidates, int32_t *membership_out,
                                    int64_t *n_components_out);
/* Nearest-neighbour lists from the same candidates: row i lists the first `top` (1 .. 1024, NOT clamped to n - 1) members of
 *     { j != i : cand(i, j) and (double)c / (double)n_hash >= threshold }   by c descending, then j ascending;
 * a row with fewer candidates is padded with index -1 / value 0.0 (count 0).  A real entry has c >= rows >= 1, so a value > 0 marks
 * exactly the real entries.  EXACT with respect to this definition; a true nearest neighbour that agrees in no whole band is missing.
 * n = 1 is valid (one row of padding).
 *
 * da_similarity_mh_lsh_knn: host boundary; idx_out int32 (n, top), val_out float64 (n, top) = c / n_hash.  Checks everything
 *   da_similarity_mh_lsh_edges_begin checks, in its order and with its texts, through max_candidates; then top outside 1 .. 1024
 *   (DA_ERR_BAD_ARG); then n_hash > 65535 (DA_ERR_UNSUPPORTED).  max_candidates as above.  da_mh_lsh_last_route reports this call too:
 *   buckets, incidences and verified pairs as above, `edges` = the real list entries written, the sum of min(candidates of row i, top).
 * da_dev_lsh_knn: the whole pipeline on resident signatures into d_idx int32 (n, top) and d_key uint16 (n, top) (the counts c; padding
 *   -1 / 0), both with leading dimension top.  d_work: da_dev_lsh_workspace_bytes(n, bands) bytes (the per-incidence and per-entry
 *   buffers are allocated inside).  Synchronises the stream.  n * bands must stay below 2^31 - 256.
 * da_dev_lsh_knn_select: the selection alone, on a caller's ragged rows: row r's entries are d_col / d_count [d_ptr[r], d_ptr[r + 1]),
 *   d_ptr int64 [n + 1], columns >= 0 and distinct within a row, in any order.  d_idx[r * ld_idx + t], d_key[r * ld_key + t] for t < top get
 *   the row's first `top` entries by (count descending, column ascending), then -1 / 0; columns >= top of the outputs are not touched.
 *   A row whose pointers run backwards or past nnz is cut to what lies inside [0, nnz): a wrong list, never an access out of bounds.
 *   Asynchronous on `stream`, no workspace. */
int da_similarity_mh_lsh_knn(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, int n_hash, const uint32_t *seeds, int bands,
                             int rows, double threshold, int top, int64_t max_candidates, int32_t *idx_out, double *val_out);
int da_dev_lsh_knn(const uint32_t *d_sig, int64_t n, int64_t ld_sig, int n_hash, int bands, int rows, double threshold, int top,
                   int64_t max_candidates, void *d_work, size_t work_bytes, int32_t *d_idx, uint16_t *d_key, void *stream);
int da_dev_lsh_knn_select(const int64_t *d_ptr, int64_t nnz, const int32_t *d_col, const uint16_t *d_count, int64_t n, int top,
                          int32_t *d_idx, int64_t ld_idx, uint16_t *d_key, int64_t ld_key, void *stream);

/* ---- MinHash LSH banding for TWO sets: a resident set y (n sequences) kept as a bucket INDEX, queried by batches x (m sequences) --------------
 * sig_x (m x n_hash) and sig_y (n x n_hash) under the same k, n_hash and seeds; bands, rows, the bands and the tail columns as above.
 * cand(i, j): some band of sig_x[i] equals the same band of sig_y[j] in all its columns; c(i, j) = the equal columns over all n_hash.
 *   edges:  (i, j, c / n_hash) for 0 <= i < m, 0 <= j < n with cand(i, j) and (double)c / (double)n_hash >= threshold, sorted by (i, j).
 *           No diagonal (i and j number different sets); every weight is > 0 (c >= rows >= 1).  Exactly the entries (i, j - m) with
 *           i < m <= j of the one-set edge list of the stacked signatures [sig_x ; sig_y].
 *   top-k:  row i holds the first `top` (1 .. 1024, NOT clamped to n) of { j : cand(i, j), c / n_hash >= threshold } by c descending, then
 *           j ascending; the padding is index -1 / value 0.0 (count 0).
 * EXACT with respect to these definitions; approximate is only their relation to da_similarity_mh_cross_edges_begin (absolute threshold) /
 * da_similarity_mh_cross_topk: a pair that agrees in no whole band is missing, with probability (1 - s^rows)^bands at similarity s.
 *
 * The index of y: its (band key, id) elements -- the keys of da_dev_lsh_band_keys -- in one stable sort, so equal keys keep their ids
 * ascending.  It lives in ONE caller-owned device buffer of da_dev_lsh_index_bytes(n, bands) bytes, depends on nothing but sig_y, bands and
 * rows, is only read by the query calls, and serves any number of them.  Layout, from the first 256-byte boundary at or behind d_index
 * (the size carries 256 spare bytes; a copy of the buffer must keep d_index modulo 256), every array starting on a multiple of 256 bytes
 * in this order, T = n * bands:
 *     meta        uint32[8]: 0x4C534831, n, bands, rows, the number of runs (buckets), the longest run, 0, 0
 *     band_start  uint32[bands + 1]: the elements of band t are [band_start[t], band_start[t + 1]); band_start[bands] = T
 *     keys        uint64[T], ascending: t << 48 | 48 bits of a hash of band t's values
 *     ids         int32[T]: the row of y of each element; ascending inside a run of equal keys
 * A query call given an index whose meta words are not (n, bands, rows) reads nothing else of it and returns DA_ERR_BAD_ARG.
 * m * bands and n * bands must stay below 2^31 - 256.
 *
 * da_dev_lsh_index_bytes / da_dev_lsh_cross_workspace_bytes: sizes; no device needed; > 0 for any arguments.
 * da_dev_lsh_index_build: sig_y -> d_index.  The sort's scratch is allocated inside; synchronises the stream.
 * da_dev_lsh_index_probe: the lookup alone: for element q = i * bands + t of x, d_lo[q] = the first element of the index whose key is the
 *   key of band t of sig_x[i] and d_len[q] = the length of that run -- ids[d_lo[q] .. d_lo[q] + d_len[q]) are the rows of y whose band t
 *   has that key, ascending; d_len[q] = 0 when there is none (d_lo[q] is then where the key would stand).  int32 [m * bands] each.
 *   Synchronises the stream (the index check is read back).
 * da_dev_lsh_cross_verify_pairs: the per-pair decision on LISTED triples (i, j, band), row i of sig_x against row j of sig_y:
 *   d_count[p] = c(i, j); d_keep[p] = 1 when `band` agrees in all its columns, no earlier band does, and c / n_hash >= threshold -- else 0.
 *   A triple with i outside [0, m), j outside [0, n) or a band outside [0, bands) gets 0 / 0.  Asynchronous on `stream`.
 * da_dev_lsh_cross_edges: probe, verify, emit, sort.  d_work: da_dev_lsh_cross_workspace_bytes(m, bands) bytes, any alignment (the
 *   per-incidence and per-edge buffers are sized by the data and allocated inside).  *n_edges_out = the number of edges; the first
 *   min(capacity, that) of them, in (i, j) order, go to d_i / d_j / d_count, which may be NULL when capacity is 0.  max_candidates caps the
 *   (pair, band) incidences -- the sum of the probed run lengths -- known before any pair is compared: more gives DA_ERR_UNSUPPORTED, the
 *   message naming the count, the cap and the longest probed run.  Synchronises the stream.  ld_x and ld_y are independent.
 * da_dev_lsh_cross_topk: the same through the verdicts, then the x rows' entries and da_dev_lsh_knn_select's selection into d_idx int32
 *   (m, top) and d_key uint16 (m, top) (the counts c; padding -1 / 0), both with leading dimension top.  Synchronises the stream.
 * da_similarity_mh_lsh_cross_edges_begin / da_similarity_mh_lsh_cross_topk: host boundary -- both packed sets, their signatures, the
 *   index of y and one query, in one call; the result in a da_edges handle / in idx_out int32 (m, top), val_out float64 (m, top).
 *   Checks, in this order and before any device is needed: m <= 0, n <= 0 (DA_ERR_EMPTY_INPUT), k, n_hash, NULL pointers, the offsets of x,
 *   the offsets of y; then the checks of the one-set LSH calls in their order and with their texts: bands, rows, bands * rows, the
 *   threshold, max_candidates, top (the top-k call only), n_hash > 65535.
 * da_mh_lsh_last_route reports these calls too: buckets = the runs of the index, incidences, distinct verified pairs, and the edges
 *   or real list entries written. */
size_t da_dev_lsh_index_bytes(int64_t n, int bands);
int da_dev_lsh_index_build(const uint32_t *d_sig_y, int64_t n, int64_t ld_y, int n_hash, int bands, int rows, void *d_index,
                           size_t index_bytes, void *stream);
int da_dev_lsh_index_probe(const void *d_index, size_t index_bytes, int64_t n, const uint32_t *d_sig_x, int64_t m, int64_t ld_x, int n_hash,
                           int bands, int rows, int32_t *d_lo, int32_t *d_len, void *stream);
int da_dev_lsh_cross_verify_pairs(const uint32_t *d_sig_x, int64_t m, int64_t ld_x, const uint32_t *d_sig_y, int64_t n, int64_t ld_y,
                                  int n_hash, int bands, int rows, double threshold, const int32_t *d_i, const int32_t *d_j,
                                  const int32_t *d_band, int64_t n_triples, uint16_t *d_count, uint8_t *d_keep, void *stream);
size_t da_dev_lsh_cross_workspace_bytes(int64_t m, int bands);
int da_dev_lsh_cross_edges(const void *d_index, size_t index_bytes, const uint32_t *d_sig_x, int64_t m, int64_t ld_x,
                           const uint32_t *d_sig_y, int64_t n, int64_t ld_y, int n_hash, int bands, int rows, double threshold,
                           int64_t max_candidates, void *d_work, size_t work_bytes, int32_t *d_i, int32_t *d_j, uint16_t *d_count,
                           int64_t capacity, int64_t *n_edges_out, void *stream);
int da_dev_lsh_cross_topk(const void *d_index, size_t index_bytes, const uint32_t *d_sig_x, int64_t m, int64_t ld_x,
                          const uint32_t *d_sig_y, int64_t n, int64_t ld_y, int n_hash, int bands, int rows, double threshold, int top,
                          int64_t max_candidates, void *d_work, size_t work_bytes, int32_t *d_idx, uint16_t *d_key, void *stream);
int da_similarity_mh_lsh_cross_edges_begin(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues,
                                           const int64_t *y_offsets, int64_t n, int k, int n_hash, const uint32_t *seeds, int bands,
                                           int rows, double threshold, int64_t max_candidates, da_edges **handle_out,
                                           int64_t *n_edges_out);
int da_similarity_mh_lsh_cross_topk(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues,
                                    const int64_t *y_offsets, int64_t n, int k, int n_hash, const uint32_t *seeds, int bands, int rows,
                                    double threshold, int top, int64_t max_candidates, int32_t *idx_out, double *val_out);

/* ---- NW identity on MinHash LSH candidates: the LSH filter above, the survivors scored by alignment -------------------------------------
 * The candidates are the entries of the LSH edge list at mh_threshold -- one set: every (i, i) and every i < j with cand(i, j) and
 * (double)c / (double)n_hash >= mh_threshold; two sets: every (i, j) with cand(i, j) and that count.  Every candidate, the diagonal
 * included, is aligned: x[i] as sequence1 against x[j] (two sets: y[j]) as sequence2, w = (double)matches / (double)length of the
 * reference's traceback (src/pairwiseSeqAlign.cpp:284-311).  The edge set, sorted by (i, j), 0-based:
 *     (i, j, w) for every candidate with w >= threshold and w > 0        (the rule of da_similarity_nw_cross_edges_begin)
 * -- EXACT with respect to this definition, weights bit for bit; the diagonal is not assumed to be 1.0 (with gap_open = gap_ext = 0 a
 * sequence of X against itself has w = 0.0 and no edge).  Approximate is only the definition's relation to the all-pairs NW threshold
 * graph: a pair that shares no bucket is missing.  Sequences of 1 .. 1024 residues, mixed freely: on the device every pair whose two
 * sequences have at most 127 residues takes a lane of the lane-per-pair kernel, every other one a wavefront.
 *
 * da_dev_nw_rescore_pairs: the reusable piece -- (matches, length) of ANY resident pair list over two encoded sets (da_dev_nw_encode; the
 *   same buffers twice for one set): pair p is x[d_i[p]] as sequence1 against y[d_j[p]] as sequence2, d_matches[p] / d_length[p] int32.  A
 *   pair with an index outside its set, a sequence of 0 residues or of more than 1024 gets -1 / -1.  The split by length happens on the
 *   device (classify, one exclusive sum, a stable partition; the alignment kernels are those of da_dev_nw_align_pairs and
 *   da_dev_nw_align_long_pairs without ops).  d_work: da_dev_nw_rescore_workspace_bytes(pairs, max_len, minimal) bytes, any alignment;
 *   minimal != 0 gives the smallest workspace the call takes, 0 the one that keeps up to 2^18 short pairs in flight, anything between
 *   works: a smaller workspace means more launches, never another result.  max_len is accepted for callers that know it and does not
 *   change the size today (the wavefront kernel stores nothing without ops).  0 for pairs <= 0; grows with pairs.
 *   SYNCHRONISES the stream once, between the partition and the alignments (the two class totals and the longest long sequence are
 *   read back); the alignments and the scatter into d_matches / d_length are asynchronous on `stream`.  pairs <= 2^31 - 16.
 * da_dev_lsh_nw_edges / da_dev_lsh_cross_nw_edges: the one-call device route on resident signatures and resident encoded sequences
 *   (d_codes / d_offsets of the set the signatures were made of): da_dev_lsh_edges / da_dev_lsh_cross_edges at mh_threshold, the sorted
 *   list unpacked, the rescore, the verdicts and the compaction -- nothing returns to the host in between but a few totals.  The verdict
 *   compares integers: matches >= min_matches[length], a table of 2049 int32 the host builds with the divide it uses for the weights,
 *   so 2/4 and 3/6 pass or fail together.  d_work / work_bytes: those of da_dev_lsh_edges / da_dev_lsh_cross_edges (the per-candidate
 *   buffers and the rescore workspace are sized by the data and allocated inside, the latter within DYNAALIGN_BLOCK_BYTES).  Checks:
 *   those of da_dev_lsh_edges / da_dev_lsh_cross_edges with mh_threshold as the threshold, then NULL sequence pointers, the matrix id,
 *   threshold outside [0, 1] or NaN, the outputs.  *n_edges_out = the number of edges; the first min(capacity, that) of them go to d_i /
 *   d_j / d_matches / d_length (int32; weight = (double)matches / (double)length), which may be NULL when capacity is 0.  A candidate
 *   whose pair the kernels refuse (an empty sequence, one over 1024 residues) makes the call fail with DA_ERR_UNSUPPORTED.
 *   Synchronises the stream.
 * da_similarity_nw_lsh_edges_begin / da_similarity_nw_lsh_cross_edges_begin: host boundary; the result in a da_edges handle
 *   (da_edges_fetch / da_edges_free), weights (double)matches / (double)length divided on the host.  Checks, in this order and before
 *   any device is needed: the matrix name (DA_ERR_BAD_MATRIX), as every NW entry does; then the checks of
 *   da_similarity_mh_lsh_edges_begin / da_similarity_mh_lsh_cross_edges_begin in their order and with their texts, the threshold left
 *   out -- empty input, k, n_hash, NULL pointers, offsets, bands, rows, bands * rows, max_candidates, n_hash > 65535; then the NW
 *   checks: invalid residues (DA_ERR_BAD_RESIDUE_SEQ1 / _SEQ2, the order of da_similarity_nw / da_similarity_nw_cross), an empty
 *   sequence (DA_ERR_UNSUPPORTED), a sequence over 1024 residues (DA_ERR_UNSUPPORTED); then threshold, then mh_threshold, outside
 *   [0, 1] or NaN (DA_ERR_BAD_ARG); DA_ERR_NO_DEVICE last.  max_candidates as for the MinHash calls, with their text.
 * da_nw_lsh_last_route: what the calling thread's last call of this family did -- buckets, (pair, band) incidences, distinct verified
 *   pairs, aligned pairs (the candidates, diagonal included), how many of them were short and long, and edges.  After
 *   da_dev_nw_rescore_pairs only the aligned, short and long counts are set.  NULL pointers are skipped. */
size_t da_dev_nw_rescore_workspace_bytes(int64_t pairs, int64_t max_len, int minimal);
int da_dev_nw_rescore_pairs(const uint8_t *d_x_codes, const int64_t *d_x_offsets, int64_t m, const uint8_t *d_y_codes,
                            const int64_t *d_y_offsets, int64_t n, const int32_t *d_i, const int32_t *d_j, int64_t pairs, int matrix_id,
                            int gap_open, int gap_ext, int32_t *d_matches, int32_t *d_length, void *d_work, size_t work_bytes, void *stream);
int da_dev_lsh_nw_edges(const uint32_t *d_sig, int64_t n, int64_t ld_sig, int n_hash, int bands, int rows, double mh_threshold,
                        int64_t max_candidates, const uint8_t *d_codes, const int64_t *d_offsets, int matrix_id, int gap_open, int gap_ext,
                        double threshold, void *d_work, size_t work_bytes, int32_t *d_i, int32_t *d_j, int32_t *d_matches,
                        int32_t *d_length, int64_t capacity, int64_t *n_edges_out, void *stream);
int da_dev_lsh_cross_nw_edges(const void *d_index, size_t index_bytes, const uint32_t *d_sig_x, int64_t m, int64_t ld_x,
                              const uint32_t *d_sig_y, int64_t n, int64_t ld_y, int n_hash, int bands, int rows, double mh_threshold,
                              int64_t max_candidates, const uint8_t *d_x_codes, const int64_t *d_x_offsets, const uint8_t *d_y_codes,
                              const int64_t *d_y_offsets, int matrix_id, int gap_open, int gap_ext, double threshold, void *d_work,
                              size_t work_bytes, int32_t *d_i, int32_t *d_j, int32_t *d_matches, int32_t *d_length, int64_t capacity,
                              int64_t *n_edges_out, void *stream);
int da_similarity_nw_lsh_edges_begin(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, int n_hash, const uint32_t *seeds,
                                     int bands, int rows, double mh_threshold, int64_t max_candidates, const char *matrix_name,
                                     int gap_open, int gap_ext, double threshold, da_edges **handle_out, int64_t *n_edges_out);
int da_similarity_nw_lsh_cross_edges_begin(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues,
                                           const int64_t *y_offsets, int64_t n, int k, int n_hash, const uint32_t *seeds, int bands,
                                           int rows, double mh_threshold, int64_t max_candidates, const char *matrix_name, int gap_open,
                                           int gap_ext, double threshold, da_edges **handle_out, int64_t *n_edges_out);
int da_nw_lsh_last_route(int64_t *buckets_out, int64_t *incidences_out, int64_t *verified_pairs_out, int64_t *aligned_pairs_out,
                         int64_t *short_pairs_out, int64_t *long_pairs_out, int64_t *edges_out);

/* ---- NW-ranked nearest-neighbour lists on the same candidates ---------------------------------------------------------------------------
 * One set: w{i, j} = the identity of x[min(i, j)] as sequence1 against x[max(i, j)] as sequence2 -- the value da_similarity_nw's symmetric
 * matrix holds at (i, j) and (j, i).  Row r lists the first `top` (1 .. 1024, NOT clamped to n - 1) members of
 *     { c != r : {r, c} a candidate at mh_threshold, w >= threshold and w > 0 }     by w descending, then c ascending;
 * the padding is index -1 / value 0.0, so a value > 0 marks exactly the real entries.  diag[r] = the identity of x[r] against itself,
 * scored like every other candidate, not assumed to be 1.0.  Two sets: row i of x lists { j : (i, j) a candidate, ... } with x[i] as
 * sequence1 and y[j] as sequence2; no diagonal.  The order is that of the DOUBLES: 5/10 and 10/20 tie and fall back to the column.  The
 * device orders 32-bit VALUE RANKS -- the table of da_nw_value_ranks, rank 0 = the value 0.0 -- and divides nothing; EXACT with respect
 * to this definition, values bit for bit.  Approximate is only the relation to da_similarity_nw_knn_long: a pair that shares no bucket
 * is missing.  Sequences of 1 .. 1024 residues, mixed freely.
 *
 * da_similarity_nw_lsh_knn / da_similarity_nw_lsh_cross_topk: host boundary; idx_out int32 (n, top) / (m, top), val_out float64 of the
 *   same shape, diag_out float64 [n]; val_out and diag_out may be NULL.  val = values[rank] from the table of da_nw_value_ranks(the
 *   longest sequence of the call), computed on the host as da_similarity_nw_knn_long does.  Checks, in this order and before any device
 *   is needed: those of da_similarity_nw_lsh_edges_begin / da_similarity_nw_lsh_cross_edges_begin in their order and with their texts,
 *   with top outside 1 .. 1024 (DA_ERR_BAD_ARG, the text of da_similarity_mh_lsh_knn) right behind max_candidates; DA_ERR_NO_DEVICE last.
 * da_dev_lsh_nw_knn / da_dev_lsh_cross_nw_topk: the one-call device routes on resident signatures and resident encoded sequences:
 *   da_dev_lsh_edges / da_dev_lsh_cross_edges at mh_threshold, the sorted list unpacked, da_dev_nw_rescore_pairs, the rank keys, the
 *   ragged rows (both directions of every kept pair of one set) and da_dev_nw_knn_select's selection into d_idx int32 and d_key uint32
 *   (value ranks; padding -1 / 0), both (rows, top) with leading dimension top; the one-set call also writes d_diag_key uint32 [n].
 *   d_rank: the device copy of the rank table of da_nw_value_ranks(max_len), max_len >= the longest sequence.  The kept ranks are those
 *   >= r_min, the rank of the smallest table value >= threshold, and > 0.  d_work / work_bytes: those of da_dev_lsh_edges /
 *   da_dev_lsh_cross_edges.  Nothing returns to the host in between but a few totals.  A candidate the alignment kernels refuse, or
 *   whose (matches, length) lies outside the table, makes the call fail with DA_ERR_UNSUPPORTED.  Synchronises the stream.
 * da_dev_nw_rank_keys: the rank-key step alone, on a caller's scored pair list: d_key[p] = d_rank[length * (max_len + 1) + matches]
 *   (0 when (matches, length) is outside the table: length 1 .. 2 * max_len, matches 0 .. min(length, max_len)), d_keep[p] = 1 when the key
 *   is >= r_min and > 0.  one_set != 0: a pair with i == j is not kept and its key goes to d_diag_key[i] (0 <= i < n).  d_totals uint64
 *   [2] (zeroed by the call) = the kept pairs, the pairs outside the table (-1 / -1 of a refused pair among them).  Asynchronous.
 * da_dev_nw_knn_select: the selection alone, on a caller's ragged rows, with the contract of da_dev_lsh_knn_select word for word and
 *   uint32 keys over their whole range: row r's entries are d_col / d_rank_key [d_ptr[r], d_ptr[r + 1]), d_ptr int64 [n + 1], columns
 *   >= 0 and distinct within a row, in any order.  d_idx[r * ld_idx + t], d_key[r * ld_key + t] for t < top get the row's first `top`
 *   entries by (key descending, column ascending), then -1 / 0; columns >= top of the outputs are not touched.  A row whose pointers
 *   run backwards or past nnz is cut to what lies inside [0, nnz).  Asynchronous on `stream`, no workspace.
 * da_nw_lsh_last_route reports these calls too; `edges` = the real list entries written. */
int da_similarity_nw_lsh_knn(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, int n_hash, const uint32_t *seeds, int bands,
                             int rows, double mh_threshold, int64_t max_candidates, const char *matrix_name, int gap_open, int gap_ext,
                             double threshold, int top, int32_t *idx_out, double *val_out, double *diag_out);
int da_similarity_nw_lsh_cross_topk(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues,
                                    const int64_t *y_offsets, int64_t n, int k, int n_hash, const uint32_t *seeds, int bands, int rows,
                                    double mh_threshold, int64_t max_candidates, const char *matrix_name, int gap_open, int gap_ext,
                                    double threshold, int top, int32_t *idx_out, double *val_out);
int da_dev_lsh_nw_knn(const uint32_t *d_sig, int64_t n, int64_t ld_sig, int n_hash, int bands, int rows, double mh_threshold,
                      int64_t max_candidates, const uint8_t *d_codes, const int64_t *d_offsets, int matrix_id, int gap_open, int gap_ext,
                      double threshold, int top, const uint32_t *d_rank, int max_len, void *d_work, size_t work_bytes, int32_t *d_idx,
                      uint32_t *d_key, uint32_t *d_diag_key, void *stream);
int da_dev_lsh_cross_nw_topk(const void *d_index, size_t index_bytes, const uint32_t *d_sig_x, int64_t m, int64_t ld_x,
                             const uint32_t *d_sig_y, int64_t n, int64_t ld_y, int n_hash, int bands, int rows, double mh_threshold,
                             int64_t max_candidates, const uint8_t *d_x_codes, const int64_t *d_x_offsets, const uint8_t *d_y_codes,
                             const int64_t *d_y_offsets, int matrix_id, int gap_open, int gap_ext, double threshold, int top,
                             const uint32_t *d_rank, int max_len, void *d_work, size_t work_bytes, int32_t *d_idx, uint32_t *d_key,
                             void *stream);
int da_dev_nw_rank_keys(const int32_t *d_i, const int32_t *d_j, const int32_t *d_matches, const int32_t *d_length, int64_t pairs,
                        const uint32_t *d_rank, int max_len, uint32_t r_min, int one_set, int64_t n, uint32_t *d_key, uint8_t *d_keep,
                        uint32_t *d_diag_key, uint64_t *d_totals, void *stream);
int da_dev_nw_knn_select(const int64_t *d_ptr, int64_t nnz, const int32_t *d_col, const uint32_t *d_rank_key, int64_t n, int top,
                         int32_t *d_idx, int64_t ld_idx, uint32_t *d_key, int64_t ld_key, void *stream);

/* name -> id for da_dev_nw; -1 + DA_ERR_BAD_MATRIX message when unknown. */
int da_matrix_id(const char *matrix_name);

/* Fill the strict lower triangle of an n x n device matrix from its upper
 * triangle (after a row-sharded gather of upper-triangular row blocks). */
int da_dev_symmetrize(void *d_mat, int64_t n, int64_t ld, int kind, void *stream);

/* Widen a compact uint16 block to double on the device:
 *   MH: count / n_hash      NW: (v >> 8) / (v & 255)
 * `is_nw` selects the rule; n_hash ignored for NW. */
int da_dev_widen(const uint16_t *d_in, double *d_out, int64_t count, int is_nw, int n_hash, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DYNAALIGN_H */
