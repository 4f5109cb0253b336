// nw_lsh_kernels.hip -- NW (matches, length) of a RESIDENT pair list, and the threshold list made of it (da_dev_nw_rescore_pairs,
// da_dev_lsh_nw_edges: the candidates of the LSH back end scored by alignment, nothing crossing the host in between).
//
// The listed-pair alignment kernels come in two families -- one LANE per pair for sequences of up to 127 residues (nw_align_kernels.hip),
// one WAVEFRONT per pair up to 1024 (nw_align_long_kernels.hip) -- and a resident list mixes both.  The split happens here, on the device:
//   1. k_nwl_classify: per pair both lengths from the offsets -> its class (short: both sides 1 .. 127; long: the longer side 128 .. 1024;
//      refused: an index outside its set, a length of 0 or over 1024 -- it gets -1 / -1 at once), per chunk of 64 pairs the number of
//      pairs of every class, and the longest long side (a wave maximum, then one atomic per wave).  The short pairs fall into FOUR
//      classes by the strips of 32 columns the lane-per-pair kernel works in, ceil(max(len) / 32): a wave of that kernel takes as long as
//      its longest pair, so lanes of one strip count keep each other busy (measured: profiles/r26_a_nw_lsh_edges_timing.txt).
//   2. ONE exclusive sum over [counts of class 0 per chunk ; class 1 ; ... ; long] numbers the short pairs 0 .. S - 1, strip class by
//      strip class, and the long ones S .. S + L - 1: k_nwl_partition writes (x index, y index, origin slot) there -- contiguous lists in
//      one array, each in listed order, no output atomic.  Results go back by origin slot, so they do not depend on the classes.
//   3. launch_nw_align on the first list, launch_nw_align_long on the second, both without ops: (matches, length) in list order.
//   4. k_nwl_scatter takes them back to the origin slots.
// The threshold step compares integers: the host builds min_matches[length] with the divide it uses for the weights, k_nwl_keep tests
// matches >= min_matches[length] and counts the kept per chunk, their exclusive sum places them and k_nwl_emit writes (i, j, matches,
// length) in listed order -- the order of the sorted candidate list, so nothing is sorted again.
// The nearest-neighbour lists on the same candidates (da_dev_lsh_nw_knn) order VALUES, so they leave the integers another way:
// k_nwl_rank_keys looks every (matches, length) up in the rank table of da_nw_value_ranks -- 5/10 and 10/20 get one rank -- writes the keep
// byte (rank >= r_min and rank > 0) and takes the diagonal candidates of one set aside into diag_key.  The ragged rows and the selection
// are those of the MinHash lists with a uint32 payload (lsh_kernels.hip: launch_nw_knn_entries, launch_nw_knn_select).
#include "lsh_common.hpp"

namespace da {
namespace {

constexpr int NWL_SHORT_MAX = 127, NWL_LONG_MAX = 1024;
constexpr int NWL_STRIP = 32;                                // the lane-per-pair kernel's columns per strip (AL_STRIP, nw_align_kernels.hip)
constexpr int NWL_CLASS_LONG = (NWL_SHORT_MAX + NWL_STRIP - 1) / NWL_STRIP;   // classes 0 .. 3: short pairs by ceil(max(len) / 32) - 1; 4: long
constexpr int NWL_CLASSES = NWL_CLASS_LONG + 1, NWL_CLASS_REFUSED = NWL_CLASSES;
constexpr int64_t NWL_ALIGN_PAIRS_MAX = (int64_t)1 << 18;   // pairs of the lane-per-pair kernel in flight with the full workspace (1.25 GiB)

// chunk c (64 pairs, one wave): cnt[k * (chunks + 1) + c] pairs of class k; entry `chunks` of every class stays 0, so that the exclusive
// sum holds there what lies before the next class -- the short total at the long class's first entry, everything listed at the very end
__global__ __launch_bounds__(LSH_THREADS) void k_nwl_classify(const int64_t *__restrict__ x_off, int64_t m_seqs, const int64_t *__restrict__ y_off,
                                                              int64_t n_seqs, const int32_t *__restrict__ pair_x, const int32_t *__restrict__ pair_y,
                                                              int64_t pairs, uint8_t *__restrict__ cls, long long *__restrict__ cnt,
                                                              uint32_t *__restrict__ longest, int32_t *__restrict__ matches_out,
                                                              int32_t *__restrict__ length_out) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (LSH_THREADS / 64), chunks = (pairs + 63) >> 6;
  int side_max = 0;
  for (int64_t c = (int64_t)blockIdx.x * (LSH_THREADS / 64) + (threadIdx.x >> 6); c < chunks; c += nwaves) {
    const int64_t p = c * 64 + lane;
    int k = -1;
    if (p < pairs) {
      const int64_t ix = pair_x[p], iy = pair_y[p];
      k = NWL_CLASS_REFUSED;
      if (ix >= 0 && ix < m_seqs && iy >= 0 && iy < n_seqs) {
        const int64_t l1 = x_off[ix + 1] - x_off[ix], l2 = y_off[iy + 1] - y_off[iy];
        const int64_t lo = l1 < l2 ? l1 : l2, hi = l1 < l2 ? l2 : l1;
        if (lo >= 1 && hi <= NWL_LONG_MAX) {
          k = hi <= NWL_SHORT_MAX ? ((int)hi - 1) / NWL_STRIP : NWL_CLASS_LONG;
          if (k == NWL_CLASS_LONG) side_max = max(side_max, (int)hi);
        }
      }
      cls[p] = (uint8_t)k;
      if (k == NWL_CLASS_REFUSED) { matches_out[p] = -1; length_out[p] = -1; }
    }
#pragma unroll
    for (int t = 0; t < NWL_CLASSES; ++t) {
      const unsigned long long members = __ballot(k == t);
      if (lane == 0) cnt[t * (chunks + 1) + c] = __popcll(members);
    }
  }
  for (int d = 32; d >= 1; d >>= 1) side_max = max(side_max, __shfl_xor(side_max, d));
  if (lane == 0 && side_max > 0) atomicMax(longest, (uint32_t)side_max);
}

// off = the exclusive sum of cnt: a pair of class k in chunk c goes to off[k * (chunks + 1) + c] + its rank among the chunk's pairs of
// that class (off[NWL_CLASS_LONG * (chunks + 1)] = the number of short pairs: the long list follows the short ones)
__global__ __launch_bounds__(LSH_THREADS) void k_nwl_partition(const int32_t *__restrict__ pair_x, const int32_t *__restrict__ pair_y, int64_t pairs,
                                                               const uint8_t *__restrict__ cls, const long long *__restrict__ off,
                                                               int32_t *__restrict__ list_x, int32_t *__restrict__ list_y,
                                                               int32_t *__restrict__ origin) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (LSH_THREADS / 64), chunks = (pairs + 63) >> 6;
  const unsigned long long below = (1ull << lane) - 1;
  for (int64_t c = (int64_t)blockIdx.x * (LSH_THREADS / 64) + (threadIdx.x >> 6); c < chunks; c += nwaves) {
    const int64_t p = c * 64 + lane;
    const int k = p < pairs ? (int)cls[p] : -1;
    unsigned long long mine = 0;
#pragma unroll
    for (int t = 0; t < NWL_CLASSES; ++t) {
      const unsigned long long members = __ballot(k == t);
      if (k == t) mine = members;
    }
    if (k < 0 || k >= NWL_CLASSES) continue;
    const int64_t q = (int64_t)off[k * (chunks + 1) + c] + __popcll(mine & below);
    list_x[q] = pair_x[p];
    list_y[q] = pair_y[p];
    origin[q] = (int32_t)p;
  }
}

__global__ __launch_bounds__(LSH_THREADS) void k_nwl_scatter(const int32_t *__restrict__ origin, const int32_t *__restrict__ list_matches,
                                                             const int32_t *__restrict__ list_length, int64_t count,
                                                             int32_t *__restrict__ matches_out, int32_t *__restrict__ length_out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < count; q += stride) {
    const int64_t p = origin[q];
    matches_out[p] = list_matches[q];
    length_out[p] = list_length[q];
  }
}

// 64-bit keys i << 32 | j of the sorted candidate list -> the two index lists
__global__ __launch_bounds__(LSH_THREADS) void k_nwl_split(const unsigned long long *__restrict__ key, int64_t count, int32_t *__restrict__ out_i,
                                                           int32_t *__restrict__ out_j) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += stride) {
    out_i[e] = (int32_t)(key[e] >> 32);
    out_j[e] = (int32_t)(key[e] & 0xFFFFFFFFull);
  }
}

// keep[p] = matches >= min_matches[length] (a refused pair, -1 / -1, is never kept); kept per chunk of 64 into chunk_kept[c]
__global__ __launch_bounds__(LSH_THREADS) void k_nwl_keep(const int32_t *__restrict__ matches, const int32_t *__restrict__ length, int64_t pairs,
                                                          const int32_t *__restrict__ min_matches, int table_len, uint8_t *__restrict__ keep,
                                                          long long *__restrict__ chunk_kept) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (LSH_THREADS / 64), chunks = (pairs + 63) >> 6;
  for (int64_t c = (int64_t)blockIdx.x * (LSH_THREADS / 64) + (threadIdx.x >> 6); c < chunks; c += nwaves) {
    const int64_t p = c * 64 + lane;
    bool kp = false;
    if (p < pairs) {
      const int32_t mt = matches[p], ln = length[p];
      kp = mt >= 0 && ln >= 0 && ln < table_len && mt >= min_matches[ln];
      keep[p] = kp ? 1 : 0;
    }
    const unsigned long long kept = __ballot(kp);
    if (lane == 0) chunk_kept[c] = __popcll(kept);
  }
}

__global__ __launch_bounds__(LSH_THREADS) void k_nwl_emit(const int32_t *__restrict__ pair_x, const int32_t *__restrict__ pair_y,
                                                          const int32_t *__restrict__ matches, const int32_t *__restrict__ length,
                                                          const uint8_t *__restrict__ keep, const long long *__restrict__ chunk_off, int64_t pairs,
                                                          int64_t capacity, int32_t *__restrict__ out_i, int32_t *__restrict__ out_j,
                                                          int32_t *__restrict__ out_matches, int32_t *__restrict__ out_length) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (LSH_THREADS / 64), chunks = (pairs + 63) >> 6;
  for (int64_t c = (int64_t)blockIdx.x * (LSH_THREADS / 64) + (threadIdx.x >> 6); c < chunks; c += nwaves) {
    const int64_t p = c * 64 + lane;
    const bool kp = p < pairs && keep[p] != 0;
    const unsigned long long kept = __ballot(kp);
    if (!kp) continue;
    const int64_t slot = (int64_t)chunk_off[c] + __popcll(kept & ((1ull << lane) - 1));
    if (slot >= capacity) continue;
    out_i[slot] = pair_x[p];
    out_j[slot] = pair_y[p];
    out_matches[slot] = matches[p];
    out_length[slot] = length[p];
  }
}

// key[p] = rank[length * (max_len + 1) + matches] under the domain check of k_codes_to_ranks; keep[p] = key >= r_min and key > 0.  one_set:
// a candidate with i == j is its sequence's diagonal -- its key goes to diag_key[i] (0 <= i < n_diag) and it is not kept.  totals[0] += the
// kept pairs, totals[1] += the pairs without a rank: a refused pair (-1 / -1) or a code outside the table (they get key 0 and are not kept).
__global__ __launch_bounds__(LSH_THREADS) void k_nwl_rank_keys(const int32_t *__restrict__ pair_x, const int32_t *__restrict__ pair_y,
                                                               const int32_t *__restrict__ matches, const int32_t *__restrict__ length, int64_t pairs,
                                                               const uint32_t *__restrict__ rank, int max_len, uint32_t r_min, bool one_set,
                                                               int64_t n_diag, uint32_t *__restrict__ key, uint8_t *__restrict__ keep,
                                                               uint32_t *__restrict__ diag_key, unsigned long long *__restrict__ totals) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (LSH_THREADS / 64), chunks = (pairs + 63) >> 6;
  const int64_t ml = max_len;
  unsigned long long kept_sum = 0, bad_sum = 0;
  for (int64_t c = (int64_t)blockIdx.x * (LSH_THREADS / 64) + (threadIdx.x >> 6); c < chunks; c += nwaves) {
    const int64_t p = c * 64 + lane;
    bool kp = false, bad = false;
    if (p < pairs) {
      const int64_t mt = matches[p], ln = length[p];
      uint32_t v = 0;
      if (ln >= 1 && ln <= 2 * ml && mt >= 0 && mt <= ml && mt <= ln) v = rank[ln * (ml + 1) + mt];
      else bad = true;
      const int32_t i = pair_x[p];
      if (one_set && i == pair_y[p]) {
        if (i >= 0 && i < n_diag) diag_key[i] = v;
      } else {
        kp = v >= r_min && v > 0;
      }
      key[p] = v;
      keep[p] = kp ? 1 : 0;
    }
    kept_sum += (unsigned long long)__popcll(__ballot(kp));
    bad_sum += (unsigned long long)__popcll(__ballot(bad));
  }
  if (lane == 0 && kept_sum) atomicAdd(&totals[0], kept_sum);
  if (lane == 0 && bad_sum) atomicAdd(&totals[1], bad_sum);
}

// the rescore workspace behind its first 256-byte boundary; every array starts on a multiple of 256 bytes
struct NwlLayout {
  size_t cnt, off, list_x, list_y, origin, list_matches, list_length, cls, longest, scan, scan_bytes, align;
};
NwlLayout nwl_layout(int64_t pairs) {
  const int64_t entries = NWL_CLASSES * (ceil_div(pairs, 64) + 1);
  NwlLayout l;
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t here = at; at += up256(bytes); return here; };
  l.cnt = take((size_t)entries * 8);
  l.off = take((size_t)entries * 8);
  l.list_x = take((size_t)pairs * 4);
  l.list_y = take((size_t)pairs * 4);
  l.origin = take((size_t)pairs * 4);
  l.list_matches = take((size_t)pairs * 4);
  l.list_length = take((size_t)pairs * 4);
  l.cls = take((size_t)pairs);
  l.longest = take(4);
  l.scan_bytes = scan_i64_bytes(entries);
  l.scan = take(l.scan_bytes);
  l.align = at;
  return l;
}

}  // namespace

size_t nw_rescore_fixed_bytes(int64_t pairs) { return pairs <= 0 ? 0 : nwl_layout(pairs).align + 256; }

size_t nw_rescore_workspace_bytes(int64_t pairs, bool minimal) {
  if (pairs <= 0) return 0;
  const int64_t in_flight = minimal ? 64 : std::min<int64_t>(ceil_div(pairs, 64) * 64, NWL_ALIGN_PAIRS_MAX);
  return nw_rescore_fixed_bytes(pairs) + nw_align_workspace_bytes(in_flight);
}

// (matches, length) of the listed pairs into d_matches / d_length (-1 / -1 for a refused pair); counts_host = {short, long, refused}.
// Synchronises the stream once, after the partition: the two class totals and the longest long side are read back.  What follows -- the
// alignment launches and the scatter -- is asynchronous.
int launch_nw_rescore(const uint8_t *d_x_codes, const int64_t *d_x_off, int64_t m, const uint8_t *d_y_codes, const int64_t *d_y_off, int64_t n,
                      const int32_t *d_i, const int32_t *d_j, int64_t pairs, int matrix_id, int gap_open, int gap_ext, int32_t *d_matches,
                      int32_t *d_length, void *d_work, size_t work_bytes, int64_t counts_host[3], hipStream_t stream) {
  counts_host[0] = counts_host[1] = counts_host[2] = 0;
  if (pairs <= 0) return DA_OK;
  if (pairs > 0x7ffffff0LL) return fail(DA_ERR_UNSUPPORTED, "nw rescore: %lld pairs are more than one call takes", (long long)pairs);
  if (!d_work || work_bytes < nw_rescore_workspace_bytes(pairs, true))
    return fail(DA_ERR_BAD_ARG, "nw rescore: workspace too small (%zu bytes, %zu needed)", d_work ? work_bytes : (size_t)0,
                nw_rescore_workspace_bytes(pairs, true));
  char *base = align256(static_cast<char *>(d_work));
  const size_t usable = work_bytes - (size_t)(base - static_cast<char *>(d_work));
  const NwlLayout l = nwl_layout(pairs);
  const int64_t chunks = ceil_div(pairs, 64), entries = NWL_CLASSES * (chunks + 1);
  long long *cnt = at_bytes<long long>(base, l.cnt), *off = at_bytes<long long>(base, l.off);
  int32_t *list_x = at_bytes<int32_t>(base, l.list_x), *list_y = at_bytes<int32_t>(base, l.list_y), *origin = at_bytes<int32_t>(base, l.origin);
  int32_t *list_matches = at_bytes<int32_t>(base, l.list_matches), *list_length = at_bytes<int32_t>(base, l.list_length);
  uint8_t *cls = at_bytes<uint8_t>(base, l.cls);
  uint32_t *longest = at_bytes<uint32_t>(base, l.longest);
  const dim3 grid(lsh_grid(chunks * 64)), block(LSH_THREADS);

  DA_HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)entries * 8, stream));
  DA_HIP_TRY(hipMemsetAsync(longest, 0, 4, stream));
  hipLaunchKernelGGL(k_nwl_classify, grid, block, 0, stream, d_x_off, m, d_y_off, n, d_i, d_j, pairs, cls, cnt, longest, d_matches, d_length);
  DA_HIP_TRY(hipGetLastError());
  size_t tb = l.scan_bytes;
  DA_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(at_bytes<void>(base, l.scan), tb, cnt, off, (int)entries, stream));
  hipLaunchKernelGGL(k_nwl_partition, grid, block, 0, stream, d_i, d_j, pairs, cls, off, list_x, list_y, origin);
  DA_HIP_TRY(hipGetLastError());
  long long shorts = 0, listed = 0;
  uint32_t long_max = 0;
  DA_HIP_TRY(hipMemcpyAsync(&shorts, off + NWL_CLASS_LONG * (chunks + 1), 8, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipMemcpyAsync(&listed, off + entries - 1, 8, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipMemcpyAsync(&long_max, longest, 4, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipStreamSynchronize(stream));
  const int64_t longs = (int64_t)(listed - shorts);
  if (shorts < 0 || longs < 0 || listed > pairs || (longs > 0 && (long_max <= (uint32_t)NWL_SHORT_MAX || long_max > (uint32_t)NWL_LONG_MAX)))
    return fail(DA_ERR_HIP, "nw rescore: the class totals read back are inconsistent");
  counts_host[0] = (int64_t)shorts; counts_host[1] = longs; counts_host[2] = pairs - (int64_t)listed;

  int rc;
  if ((rc = launch_nw_align(d_x_codes, d_x_off, m, d_y_codes, d_y_off, n, list_x, list_y, 0, (int64_t)shorts, matrix_id, gap_open, gap_ext, nullptr, 0,
                            list_length, list_matches, nullptr, base + l.align, usable - l.align, stream)) != DA_OK) return rc;
  if ((rc = launch_nw_align_long(d_x_codes, d_x_off, m, d_y_codes, d_y_off, n, list_x + shorts, list_y + shorts, 0, longs, matrix_id, gap_open, gap_ext,
                                 nullptr, 0, list_length + shorts, list_matches + shorts, nullptr, (int64_t)long_max, nullptr, 0, stream)) != DA_OK) return rc;
  if (listed > 0) {
    hipLaunchKernelGGL(k_nwl_scatter, dim3(lsh_grid(listed)), block, 0, stream, origin, list_matches, list_length, (int64_t)listed, d_matches, d_length);
    DA_HIP_TRY(hipGetLastError());
  }
  return DA_OK;
}

int launch_nwl_split(const uint64_t *d_key, int64_t count, int32_t *d_i, int32_t *d_j, hipStream_t stream) {
  if (count <= 0) return DA_OK;
  hipLaunchKernelGGL(k_nwl_split, dim3(lsh_grid(count)), dim3(LSH_THREADS), 0, stream, reinterpret_cast<const unsigned long long *>(d_key), count, d_i, d_j);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

// d_totals (two words, zeroed here): the kept pairs and the pairs without a rank; d_diag_key may be NULL when one_set is false
int launch_nwl_rank_keys(const int32_t *d_i, const int32_t *d_j, const int32_t *d_matches, const int32_t *d_length, int64_t pairs, const uint32_t *d_rank,
                         int max_len, uint32_t r_min, bool one_set, int64_t n_diag, uint32_t *d_key, uint8_t *d_keep, uint32_t *d_diag_key,
                         uint64_t *d_totals, hipStream_t stream) {
  DA_HIP_TRY(hipMemsetAsync(d_totals, 0, 16, stream));
  if (pairs <= 0) return DA_OK;
  hipLaunchKernelGGL(k_nwl_rank_keys, dim3(lsh_grid(ceil_div(pairs, 64) * 64)), dim3(LSH_THREADS), 0, stream, d_i, d_j, d_matches, d_length, pairs, d_rank,
                     max_len, r_min, one_set, n_diag, d_key, d_keep, d_diag_key, reinterpret_cast<unsigned long long *>(d_totals));
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

size_t nwl_keep_scan_bytes(int64_t pairs) { return up256(scan_i64_bytes(ceil_div(pairs, 64) + 1)) + 256; }

// the verdicts (d_keep, one per pair), the kept per chunk of 64 (d_chunk_kept: chunks + 1 entries, the last one 0) and their exclusive
// sum (d_chunk_off: its last entry is the number of kept pairs); d_min_matches: table_len int32 on the device
int launch_nwl_keep(const int32_t *d_matches, const int32_t *d_length, int64_t pairs, const int32_t *d_min_matches, int table_len, uint8_t *d_keep,
                    int64_t *d_chunk_kept, int64_t *d_chunk_off, void *d_temp, size_t temp_bytes, hipStream_t stream) {
  const int64_t chunks = ceil_div(pairs, 64);
  DA_HIP_TRY(hipMemsetAsync(d_chunk_kept + chunks, 0, 8, stream));
  if (pairs > 0) {
    hipLaunchKernelGGL(k_nwl_keep, dim3(lsh_grid(chunks * 64)), dim3(LSH_THREADS), 0, stream, d_matches, d_length, pairs, d_min_matches, table_len, d_keep,
                       reinterpret_cast<long long *>(d_chunk_kept));
    DA_HIP_TRY(hipGetLastError());
  }
  void *temp = align256(static_cast<char *>(d_temp));
  size_t tb = temp_bytes - 256;
  DA_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(temp, tb, reinterpret_cast<const long long *>(d_chunk_kept), reinterpret_cast<long long *>(d_chunk_off),
                                              (int)(chunks + 1), stream));
  return DA_OK;
}

// the kept pairs at their final positions, the first `capacity` of them
int launch_nwl_emit(const int32_t *d_i, const int32_t *d_j, const int32_t *d_matches, const int32_t *d_length, const uint8_t *d_keep,
                    const int64_t *d_chunk_off, int64_t pairs, int64_t capacity, int32_t *d_out_i, int32_t *d_out_j, int32_t *d_out_matches,
                    int32_t *d_out_length, hipStream_t stream) {
  if (pairs <= 0 || capacity <= 0) return DA_OK;
  hipLaunchKernelGGL(k_nwl_emit, dim3(lsh_grid(ceil_div(pairs, 64) * 64)), dim3(LSH_THREADS), 0, stream, d_i, d_j, d_matches, d_length, d_keep,
                     reinterpret_cast<const long long *>(d_chunk_off), pairs, capacity, d_out_i, d_out_j, d_out_matches, d_out_length);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

}  // namespace da
