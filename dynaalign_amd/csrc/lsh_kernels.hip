// lsh_kernels.hip -- MinHash LSH banding: the threshold graph of one set without the n x n compare, and the BACK END of both LSH forms.
// The n_hash columns of a signature are cut into `bands` bands of `rows` columns; two sequences are a CANDIDATE when some band agrees in
// all its columns, and only candidates are compared.  The result is exact with respect to that definition (lsh_edges_dense in
// similarity.py): a bucket key is a hash, but a pair becomes an edge only after the band's columns were compared themselves.
//
// A front end numbers the (pair, band) INCIDENCES as the slots of an exclusive sum and describes them in an LshSlots (da_common.hpp).
// Steps 1 and 2 below are the one-set front end; the two-set one -- a resident index and its probe -- is lsh_cross_kernels.hip.  Steps 3
// and 4 and the nearest-neighbour lists further down are the back end: row i of sig_a against row j of sig_b, which the one-set form
// passes the same matrix for.
//
//   1. k_lsh_band_keys: element q = i * bands + t  ->  key = band t in the top 16 bits | 48 bits of a hash of the band's values, id = i;
//   2. one stable hipcub radix sort of (key, id): a bucket is a run of equal keys, never spans two bands, and holds its ids ascending, so
//      every enumerated pair already has i < j.  k_lsh_run_heads / an inclusive sum / k_lsh_run_starts / k_lsh_partner_counts give each
//      element p of a run ending at e its e - 1 - p partners; their exclusive sum numbers the (pair, band) INCIDENCES, and its total is known
//      -- and checked against the caller's cap -- before any pair is touched;
//   3. k_lsh_verify, the hot kernel: a wave takes 64 consecutive incidence slots, every lane finds its slot's (i, j, band) (a binary search
//      of the exclusive sum: balanced whatever the bucket sizes are; LshEnumerated for one set, LshProbed for two), then the wave decides
//      the 64 pairs one after the other with lsh_pair_decide -- both signature rows read coalesced, equal columns counted by ballot /
//      popcount.  A pair survives in the FIRST band in which it agrees only (exact deduplication without a sort of candidates) and when
//      its count reaches c_min.  Per chunk of 64 slots the kept count; their scan; k_lsh_emit writes i << 32 | j and the count into final
//      slots -- no output atomic;
//   4. one radix sort of the 64-bit keys (count as payload) puts the list in (i, j) order -- behind the n diagonal entries of one set; two
//      sets have no diagonal, i and j number different sets -- and k_lsh_split unpacks it.
// The same verify kernel runs on LISTED triples (da_dev_lsh_verify_pairs, da_dev_lsh_cross_verify_pairs), so that the per-pair decision
// can be tested on triples the pipeline never produces (a key collision, a pair of an earlier band).
#include "components_common.hpp"
#include "lsh_common.hpp"
#include "scan.hpp"

namespace da {
namespace {

// Consecutive threads take consecutive bands of one row: a wave reads one stretch of the row and writes one stretch of keys / ids.
// Only columns < bands * rows are read.
__global__ __launch_bounds__(LSH_THREADS) void k_lsh_band_keys(const uint32_t *__restrict__ sig, int64_t ld_sig, int64_t total, int bands, int rows,
                                                               unsigned long long *__restrict__ keys, int32_t *__restrict__ ids) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += stride) {
    const int64_t i = q / bands;
    const int t = (int)(q - i * bands);
    keys[q] = lsh_band_key(sig + i * ld_sig + (int64_t)t * rows, rows, t);
    ids[q] = (int32_t)i;
  }
}

__global__ __launch_bounds__(LSH_THREADS) void k_lsh_run_heads(const unsigned long long *__restrict__ keys, int64_t total, uint32_t *__restrict__ head) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += stride) head[p] = (p == 0 || keys[p] != keys[p - 1]) ? 1u : 0u;
}

// run_no[p] = the inclusive sum of head[]: the 1-based number of p's run.  start[r] = first element of run r (0-based), start[runs] = total.
__global__ __launch_bounds__(LSH_THREADS) void k_lsh_run_starts(const uint32_t *__restrict__ head, const uint32_t *__restrict__ run_no, int64_t total,
                                                                uint32_t *__restrict__ start) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += stride) {
    if (head[p]) start[run_no[p] - 1] = (uint32_t)p;
    if (p == total - 1) start[run_no[p]] = (uint32_t)total;
  }
}

// cnt[p] = e - 1 - p for the run [.., e) of p; cnt[total] = 0 (so that the exclusive sum ends with the total).
// stats[0] = the largest run (a maximum, taken per wave first), stats[1] = the number of runs.
__global__ __launch_bounds__(LSH_THREADS) void k_lsh_partner_counts(const uint32_t *__restrict__ run_no, const uint32_t *__restrict__ start, int64_t total,
                                                                    long long *__restrict__ cnt, uint32_t *__restrict__ stats) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  uint32_t longest = 0;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p <= total; p += stride) {
    if (p == total) { cnt[p] = 0; continue; }
    const uint32_t r = run_no[p], e = start[r];
    cnt[p] = (long long)e - 1 - p;
    longest = max(longest, e - start[r - 1]);
    if (p == total - 1) stats[1] = r;
  }
  for (int o = 32; o > 0; o >>= 1) longest = max(longest, (uint32_t)__shfl_down(longest, o));
  if ((threadIdx.x & 63) == 0 && longest) atomicMax(&stats[0], longest);
}

// ---- where the triples of the verify kernel come from: lane-level get(slot) ----------------------------------------------------------------
struct LshListed {
  const int32_t *__restrict__ i, *__restrict__ j, *__restrict__ band;
  __device__ __forceinline__ void get(int64_t s, int &pi, int &pj, int &pt) const { pi = i[s]; pj = j[s]; pt = band[s]; }
};
// one set: slot s of the exclusive sum off[0 .. total] of the partner counts: the element p with off[p] <= s < off[p + 1] and its partner
// p + 1 + (s - off[p])
struct LshEnumerated {
  const long long *__restrict__ off;
  const int32_t *__restrict__ ids;
  const unsigned long long *__restrict__ keys;
  int64_t total;
  __device__ __forceinline__ void get(int64_t s, int &pi, int &pj, int &pt) const {
    int64_t lo = 0, hi = total;                          // the last p with off[p] <= s (s < off[total], so p < total)
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (off[mid] <= s) lo = mid; else hi = mid - 1;
    }
    pi = ids[lo];
    pj = ids[lo + 1 + (s - off[lo])];
    pt = (int)(keys[lo] >> LSH_BAND_SHIFT);
  }
};
// two sets: slot s of the exclusive sum off[0 .. elements] of the probed lengths: the element q with off[q] <= s < off[q + 1] (the LAST q
// with off[q] <= s: the elements of length 0 behind it share its successor's offset) and member s - off[q] of its run
struct LshProbed {
  const long long *__restrict__ off;
  const uint32_t *__restrict__ lo;
  const int32_t *__restrict__ ids;
  int64_t elements;
  int bands;
  __device__ __forceinline__ void get(int64_t s, int &pi, int &pj, int &pt) const {
    int64_t a = 0, b = elements;                         // s < off[elements], so the answer is < elements
    while (a < b) {
      const int64_t mid = (a + b + 1) >> 1;
      if (off[mid] <= s) a = mid; else b = mid - 1;
    }
    pi = (int)(a / bands);
    pt = (int)(a - (int64_t)pi * bands);
    pj = ids[(int64_t)lo[a] + (s - off[a])];
  }
};
// the one place where a launcher learns which enumeration the slots hold: f(the device-side source)
template <typename F> void with_source(const LshSlots &s, F f) {
  const long long *off = reinterpret_cast<const long long *>(s.off);
  if (s.probed) f(LshProbed{off, s.lo, s.ids, s.elements, s.bands});
  else f(LshEnumerated{off, s.ids, reinterpret_cast<const unsigned long long *>(s.keys), s.elements});
}

// Row i of sig_a against row j of sig_b.  out_count[s] = the pair's count, out_keep[s] = 1 when the triple survives.  A triple with i
// outside [0, rows_a), j outside [0, rows_b) or a band outside [0, bands) reads nothing and gets 0 / 0.  chunk_kept[c] (if given) = kept
// triples of slots [64 c, 64 c + 64); *distinct (if given) += the triples that are their pair's first agreeing band, whatever their count.
template <typename Src>
__global__ __launch_bounds__(LSH_THREADS) void k_lsh_verify(const uint32_t *__restrict__ sig_a, int64_t rows_a, int64_t ld_a,
                                                            const uint32_t *__restrict__ sig_b, int64_t rows_b, int64_t ld_b, int n_hash, int bands, int rows,
                                                            uint32_t c_min, Src src, int64_t slots, uint16_t *__restrict__ out_count,
                                                            uint8_t *__restrict__ out_keep, long long *__restrict__ chunk_kept,
                                                            unsigned long long *__restrict__ distinct) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (LSH_THREADS / 64), chunks = (slots + 63) >> 6;
  unsigned long long firsts = 0;
  for (int64_t c = (int64_t)blockIdx.x * (LSH_THREADS / 64) + (threadIdx.x >> 6); c < chunks; c += nwaves) {
    const int64_t s = c * 64 + lane;
    int i = 0, j = 0, t = 0;
    bool valid = false;
    if (s < slots) {
      src.get(s, i, j, t);
      valid = i >= 0 && i < rows_a && j >= 0 && j < rows_b && t >= 0 && t < bands;
    }
    unsigned long long todo = __ballot(valid);
    uint32_t my_count = 0;
    bool my_first = false;
    while (todo) {
      const int b = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int bi = __shfl(i, b), bj = __shfl(j, b), bt = __shfl(t, b);
      const LshVerdict v = lsh_pair_decide(sig_a + (int64_t)bi * ld_a, sig_b + (int64_t)bj * ld_b, n_hash, bands * rows, rows, bt);
      if (lane == b) { my_count = v.count; my_first = v.first; }
    }
    const bool keep = my_first && my_count >= c_min;
    if (s < slots) { out_count[s] = (uint16_t)my_count; out_keep[s] = keep ? 1 : 0; }
    const unsigned long long kept = __ballot(keep);
    if (chunk_kept && lane == 0) chunk_kept[c] = __popcll(kept);
    firsts += (unsigned long long)__popcll(__ballot(my_first));
  }
  if (distinct && lane == 0 && firsts) atomicAdd(distinct, firsts);
}

// the kept slots of chunk c, in slot order, at edge slots base + chunk_off[c] ...: key = i << 32 | j, value = the count
template <typename Src>
__global__ __launch_bounds__(LSH_THREADS) void k_lsh_emit(Src src, int64_t slots, const uint16_t *__restrict__ count, const uint8_t *__restrict__ keep,
                                                          const long long *__restrict__ chunk_off, int64_t base, unsigned long long *__restrict__ out_key,
                                                          uint16_t *__restrict__ out_val) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (LSH_THREADS / 64), chunks = (slots + 63) >> 6;
  for (int64_t c = (int64_t)blockIdx.x * (LSH_THREADS / 64) + (threadIdx.x >> 6); c < chunks; c += nwaves) {
    const int64_t s = c * 64 + lane;
    const bool kp = s < slots && keep[s] != 0;
    const unsigned long long kept = __ballot(kp);
    if (!kp) continue;
    int i, j, t;
    src.get(s, i, j, t);
    const int64_t slot = base + chunk_off[c] + __popcll(kept & ((1ull << lane) - 1));
    out_key[slot] = ((unsigned long long)(uint32_t)i << 32) | (uint32_t)j;
    out_val[slot] = count[s];
  }
}

// The components tail (da_dev_lsh_components): the same slot enumeration as k_lsh_emit, but a kept slot is not written anywhere -- its pair
// goes through the union step of components_common.hpp.  No chunk offsets, no 64-bit keys, no sort.  One set only: i and j number the
// same vertices.
template <typename Src>
__global__ __launch_bounds__(LSH_THREADS) void k_lsh_union(Src src, int64_t slots, const uint8_t *__restrict__ keep, int32_t *parent) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (LSH_THREADS / 64), chunks = (slots + 63) >> 6;
  for (int64_t c = (int64_t)blockIdx.x * (LSH_THREADS / 64) + (threadIdx.x >> 6); c < chunks; c += nwaves) {
    const int64_t s = c * 64 + lane;
    if (s >= slots || keep[s] == 0) continue;
    int i, j, t;
    src.get(s, i, j, t);
    cc_union(parent, i, j);                       // a kept slot was valid in k_lsh_verify: 0 <= i < j < n
  }
}

__global__ __launch_bounds__(LSH_THREADS) void k_lsh_diagonal(int64_t n, int n_hash, unsigned long long *__restrict__ out_key, uint16_t *__restrict__ out_val) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    out_key[i] = ((unsigned long long)i << 32) | (unsigned long long)i;
    out_val[i] = (uint16_t)n_hash;
  }
}

__global__ __launch_bounds__(LSH_THREADS) void k_lsh_split(const unsigned long long *__restrict__ key, const uint16_t *__restrict__ val, int64_t count,
                                                           int32_t *__restrict__ out_i, int32_t *__restrict__ out_j, uint16_t *__restrict__ out_count) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += stride) {
    out_i[e] = (int32_t)(key[e] >> 32);
    out_j[e] = (int32_t)(key[e] & 0xFFFFFFFFull);
    out_count[e] = val[e];
  }
}

// the bucket workspace of `total` = n * bands elements, cut into its arrays
struct BucketLayout {
  size_t keys_in, keys_out, ids_in, ids_out, start, cnt, off, stats, temp, temp_bytes, bytes;
  explicit BucketLayout(int64_t total) {
    const size_t t = (size_t)total;
    size_t at = 0;
    auto take = [&](size_t b) { const size_t o = at; at += up256(b); return o; };
    keys_in = take(t * 8);        // after the sort: head[] and run_no[] (uint32 each)
    keys_out = take(t * 8);
    ids_in = take(t * 4);
    ids_out = take(t * 4);
    start = take((t + 1) * 4);
    cnt = take((t + 1) * 8);
    off = take((t + 1) * 8);
    stats = take(16);
    temp_bytes = std::max(std::max(sort_u64_i32_bytes(total), scan_u32_bytes(total)), scan_i64_bytes(total + 1));
    temp = take(temp_bytes);
    bytes = at + 256;
  }
};

}  // namespace

int launch_lsh_band_keys(const uint32_t *d_sig, int64_t n, int64_t ld_sig, int bands, int rows, uint64_t *d_keys, int32_t *d_ids, hipStream_t stream) {
  const int64_t total = n * bands;
  if (total <= 0) return DA_OK;
  hipLaunchKernelGGL(k_lsh_band_keys, dim3(lsh_grid(total)), dim3(LSH_THREADS), 0, stream, d_sig, ld_sig, total, bands, rows,
                     reinterpret_cast<unsigned long long *>(d_keys), d_ids);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

size_t lsh_workspace_bytes(int64_t n, int bands) {
  if (n <= 0 || bands <= 0 || n * (int64_t)bands > LSH_MAX_ELEMENTS) return 256;
  return BucketLayout(n * bands).bytes;
}

// Steps 1 and 2 on the signatures: keys, the sort, the runs, the partner counts and their exclusive sum.  The slots point into the
// workspace; stats_host = {largest bucket, buckets}, *incidences_host the total; synchronises the stream once (the read-back).
int lsh_buckets(const uint32_t *d_sig, int64_t n, int64_t ld_sig, int bands, int rows, void *d_work, size_t work_bytes, LshSlots *slots_out,
                uint32_t stats_host[2], int64_t *incidences_host, hipStream_t stream) {
  const int64_t total = n * bands;
  const BucketLayout L(total);
  if (!d_work || work_bytes < L.bytes) return fail(DA_ERR_BAD_ARG, "lsh: workspace too small (%zu bytes, %zu needed)", work_bytes, L.bytes);
  // the arrays start on 256 bytes whatever the caller's pointer: the layout's 256 spare bytes are for this
  d_work = static_cast<char *>(d_work) + ((256 - (reinterpret_cast<uintptr_t>(d_work) & 255)) & 255);
  unsigned long long *keys_in = at_bytes<unsigned long long>(d_work, L.keys_in), *keys_out = at_bytes<unsigned long long>(d_work, L.keys_out);
  int32_t *ids_in = at_bytes<int32_t>(d_work, L.ids_in), *ids_out = at_bytes<int32_t>(d_work, L.ids_out);
  uint32_t *head = at_bytes<uint32_t>(d_work, L.keys_in), *run_no = head + total;
  uint32_t *start = at_bytes<uint32_t>(d_work, L.start), *stats = at_bytes<uint32_t>(d_work, L.stats);
  long long *cnt = at_bytes<long long>(d_work, L.cnt), *off = at_bytes<long long>(d_work, L.off);
  void *temp = at_bytes<char>(d_work, L.temp);
  int rc;
  if ((rc = launch_lsh_band_keys(d_sig, n, ld_sig, bands, rows, reinterpret_cast<uint64_t *>(keys_in), ids_in, stream)) != DA_OK) return rc;
  size_t tb = L.temp_bytes;
  DA_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(temp, tb, keys_in, keys_out, ids_in, ids_out, (int)total, 0, LSH_BAND_SHIFT + bits_for(bands), stream));
  const unsigned grid = lsh_grid(total + 1);
  hipLaunchKernelGGL(k_lsh_run_heads, dim3(grid), dim3(LSH_THREADS), 0, stream, keys_out, total, head);
  DA_HIP_TRY(hipGetLastError());
  tb = L.temp_bytes;
  DA_HIP_TRY(hipcub::DeviceScan::InclusiveSum(temp, tb, head, run_no, (int)total, stream));
  hipLaunchKernelGGL(k_lsh_run_starts, dim3(grid), dim3(LSH_THREADS), 0, stream, head, run_no, total, start);
  DA_HIP_TRY(hipGetLastError());
  DA_HIP_TRY(hipMemsetAsync(stats, 0, 16, stream));
  hipLaunchKernelGGL(k_lsh_partner_counts, dim3(grid), dim3(LSH_THREADS), 0, stream, run_no, start, total, cnt, stats);
  DA_HIP_TRY(hipGetLastError());
  tb = L.temp_bytes;
  DA_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(temp, tb, cnt, off, (int)(total + 1), stream));
  long long inc = 0;
  DA_HIP_TRY(hipMemcpyAsync(&inc, off + total, 8, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipMemcpyAsync(stats_host, stats, 8, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipStreamSynchronize(stream));
  *incidences_host = (int64_t)inc;
  *slots_out = LshSlots{false, reinterpret_cast<const int64_t *>(off), ids_out, reinterpret_cast<const uint64_t *>(keys_out), nullptr, total, bands};
  return DA_OK;
}

int launch_lsh_verify_listed(const uint32_t *d_sig_a, int64_t rows_a, int64_t ld_a, const uint32_t *d_sig_b, int64_t rows_b, int64_t ld_b, int n_hash,
                             int bands, int rows, uint32_t c_min, const int32_t *d_i, const int32_t *d_j, const int32_t *d_band, int64_t triples,
                             uint16_t *d_count, uint8_t *d_keep, hipStream_t stream) {
  if (triples <= 0) return DA_OK;
  hipLaunchKernelGGL(k_lsh_verify<LshListed>, dim3(lsh_grid(ceil_div(triples, 64) * 64)), dim3(LSH_THREADS), 0, stream, d_sig_a, rows_a, ld_a, d_sig_b,
                     rows_b, ld_b, n_hash, bands, rows, c_min, LshListed{d_i, d_j, d_band}, triples, d_count, d_keep, (long long *)nullptr,
                     (unsigned long long *)nullptr);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

// scratch of the scan over the chunk counts of `incidences` slots
size_t lsh_chunk_scan_bytes(int64_t incidences) { return up256(scan_i64_bytes(ceil_div(incidences, 64) + 1)) + 256; }

// Step 3 on the enumerated incidences: verdicts into d_count / d_keep (one per incidence), kept counts per chunk of 64 into d_chunk_kept
// (chunks + 1 entries, the last one 0), their exclusive sum into d_chunk_off (d_temp: lsh_chunk_scan_bytes(incidences)); *d_distinct
// (zeroed here) counts the distinct candidate pairs.
int launch_lsh_verify_enumerated(const uint32_t *d_sig_a, int64_t rows_a, int64_t ld_a, const uint32_t *d_sig_b, int64_t rows_b, int64_t ld_b, int n_hash,
                                 int rows, uint32_t c_min, const LshSlots &slots, int64_t incidences, uint16_t *d_count, uint8_t *d_keep,
                                 int64_t *d_chunk_kept, int64_t *d_chunk_off, uint64_t *d_distinct, void *d_temp, size_t temp_bytes, hipStream_t stream) {
  const int64_t chunks = ceil_div(incidences, 64);
  DA_HIP_TRY(hipMemsetAsync(d_distinct, 0, 8, stream));
  DA_HIP_TRY(hipMemsetAsync(d_chunk_kept + chunks, 0, 8, stream));
  if (incidences > 0) {
    with_source(slots, [&](auto src) {
      hipLaunchKernelGGL(k_lsh_verify<decltype(src)>, dim3(lsh_grid(chunks * 64)), dim3(LSH_THREADS), 0, stream, d_sig_a, rows_a, ld_a, d_sig_b, rows_b, ld_b,
                         n_hash, slots.bands, rows, c_min, src, incidences, d_count, d_keep, reinterpret_cast<long long *>(d_chunk_kept),
                         reinterpret_cast<unsigned long long *>(d_distinct));
    });
    DA_HIP_TRY(hipGetLastError());
  }
  size_t tb = temp_bytes;
  DA_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_temp, tb, reinterpret_cast<const long long *>(d_chunk_kept), reinterpret_cast<long long *>(d_chunk_off),
                                              (int)(chunks + 1), stream));
  return DA_OK;
}

size_t lsh_edge_sort_bytes(int64_t edges) { return up256(sort_u64_u16_bytes(edges)) + 256; }

// Step 3's emit and step 4: the diagonal_n diagonal entries (one set: its rows; two sets: 0) and the kept incidences into d_key_in /
// d_val_in (edges = diagonal_n + kept entries, > 0), sorted by (i, j) into d_key_out / d_val_out (d_temp: lsh_edge_sort_bytes(edges)).
// rows_a = the range of i.
int launch_lsh_emit_sort(const LshSlots &slots, int64_t rows_a, int64_t diagonal_n, int n_hash, int64_t incidences, const uint16_t *d_count,
                         const uint8_t *d_keep, const int64_t *d_chunk_off, int64_t edges, uint64_t *d_key_in, uint16_t *d_val_in, uint64_t *d_key_out,
                         uint16_t *d_val_out, void *d_temp, size_t temp_bytes, hipStream_t stream) {
  unsigned long long *kin = reinterpret_cast<unsigned long long *>(d_key_in), *kout = reinterpret_cast<unsigned long long *>(d_key_out);
  if (diagonal_n > 0) {
    hipLaunchKernelGGL(k_lsh_diagonal, dim3(lsh_grid(diagonal_n)), dim3(LSH_THREADS), 0, stream, diagonal_n, n_hash, kin, d_val_in);
    DA_HIP_TRY(hipGetLastError());
  }
  if (incidences > 0 && edges > diagonal_n) {
    with_source(slots, [&](auto src) {
      hipLaunchKernelGGL(k_lsh_emit<decltype(src)>, dim3(lsh_grid(ceil_div(incidences, 64) * 64)), dim3(LSH_THREADS), 0, stream, src, incidences, d_count,
                         d_keep, reinterpret_cast<const long long *>(d_chunk_off), diagonal_n, kin, d_val_in);
    });
    DA_HIP_TRY(hipGetLastError());
  }
  size_t tb = temp_bytes;
  DA_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(d_temp, tb, kin, kout, d_val_in, d_val_out, (int)edges, 0, 32 + bits_for(rows_a), stream));
  return DA_OK;
}

// the union step over the kept slots of launch_lsh_verify_enumerated, into the parent array of launch_cc_init (one set: rows_a vertices)
int launch_lsh_union(const LshSlots &slots, int64_t incidences, const uint8_t *d_keep, int32_t *d_parent, hipStream_t stream) {
  if (incidences <= 0) return DA_OK;
  if (slots.probed) return fail(DA_ERR_UNSUPPORTED, "lsh: components of two sets are not defined");
  const unsigned grid = std::min<unsigned>(lsh_grid(ceil_div(incidences, 64) * 64), (unsigned)components_max_blocks());
  with_source(slots, [&](auto src) {
    hipLaunchKernelGGL(k_lsh_union<decltype(src)>, dim3(grid), dim3(LSH_THREADS), 0, stream, src, incidences, d_keep,
                       d_parent);
  });
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

int launch_lsh_split(const uint64_t *d_key, const uint16_t *d_val, int64_t count, int32_t *d_i, int32_t *d_j, uint16_t *d_count, hipStream_t stream) {
  if (count <= 0) return DA_OK;
  hipLaunchKernelGGL(k_lsh_split, dim3(lsh_grid(count)), dim3(LSH_THREADS), 0, stream, reinterpret_cast<const unsigned long long *>(d_key), d_val, count,
                     d_i, d_j, d_count);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

// ---- nearest-neighbour lists from the candidates (da_dev_lsh_knn, da_dev_lsh_knn_select) --------------------------------------------------
// After step 3 every kept slot is a distinct pair with its count.  Row i's list is the first `top` of its candidates by (count descending,
// column ascending).  One set has i < j in every slot, so both directions of a pair are needed (BOTH); two sets list the rows of x only:
//   5. k_lsh_knn_entries<Src, V, false, BOTH> (V: the payload -- the uint16 count here, the uint32 value rank of the NW lists): deg[i]++ and,
//      with BOTH, deg[j]++ over the kept slots; an exclusive sum gives ptr[rows + 1];
//   6. k_lsh_knn_entries<Src, V, true, BOTH>: (col = j, count) into row i's segment and, with BOTH, (col = i, count) into row j's, through a
//      per-row cursor.  The slots of a chunk mostly share their i (the partners of one element, the run of one x row, are consecutive
//      slots), so the i side takes ONE atomic per distinct i of the chunk and writes its entries side by side; the j side takes one atomic
//      per entry.  The order inside a segment is whatever the scheduling gives: the selection does not depend on it;
//   7. the selection, on the words (KEY_MAX - key) << 32 | col -- ascending word order is key descending, column ascending, and the words
//      of a row are distinct because its columns are.  The key is the uint16 count (a 48-bit word, six radix digits) or, for the NW lists
//      on the same candidates (da_dev_nw_knn_select, nw_lsh_kernels.hip), a uint32 value rank (the full 64-bit word, eight digits): one
//      template, KnnKey<K> holds what differs.  Degrees are very skewed, so there are two kernels:
//        k_lsh_knn_select_short  rows of up to LSH_KNN_WAVE_MAX entries: a wave per row, an entry per lane, a bitonic sort by shuffles;
//        k_lsh_knn_select_long   the other rows: a workgroup looks at LSH_KNN_TILE rows at a time, lists the long ones in LDS and takes them
//                                one after the other.  Up to LSH_KNN_LDS_WORDS entries are loaded and sorted whole in LDS.  A longer row
//                                first finds T, its top-th smallest word, by an MSD radix select over the word's 8-bit digits (a 256-bin LDS
//                                histogram per digit, over the entries that match the digits fixed so far), then compacts the words
//                                <= T -- exactly `top` of them -- through an LDS counter and sorts those.
//      Neither kernel needs a workspace, so the selection on a caller's ragged rows is asynchronous.
namespace {
constexpr int LSH_KNN_WAVE_MAX = 64;
constexpr int LSH_KNN_LDS_WORDS = 2048;
constexpr int LSH_KNN_TILE = LSH_THREADS;
static_assert(DA_TOPK_MAX <= LSH_KNN_LDS_WORDS, "the candidates of the radix path are sorted in the same buffer");

__device__ __forceinline__ unsigned long long lsh_shfl_xor64(unsigned long long v, int mask) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, mask), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), mask);
  return ((unsigned long long)hi << 32) | lo;
}
// what the two key types of the selection differ in: the largest key and the 8-bit digits of the word (KEY_MAX - key) << 32 | column
template <typename K> struct KnnKey;
template <> struct KnnKey<uint16_t> { static constexpr unsigned long long MAX = 0xFFFFull; static constexpr int DIGITS = 6; };
template <> struct KnnKey<uint32_t> { static constexpr unsigned long long MAX = 0xFFFFFFFFull; static constexpr int DIGITS = 8; };
template <typename K> __device__ __forceinline__ unsigned long long lsh_knn_word(int32_t col, K key) {
  return ((KnnKey<K>::MAX - (unsigned long long)key) << 32) | (uint32_t)col;
}
// row r's entries: [b, e), with a pointer that runs backwards or past nnz cut to what lies inside [0, nnz)
__device__ __forceinline__ void lsh_knn_segment(const long long *__restrict__ ptr, int64_t r, int64_t nnz, int64_t &b, int64_t &e) {
  b = min(max((int64_t)ptr[r], (int64_t)0), nnz);
  e = min(max((int64_t)ptr[r + 1], (int64_t)0), nnz);
  if (e < b) e = b;
}

// SCATTER = false: at[] are the degrees.  SCATTER = true: at[] are the cursors (they start as the row pointers) and the entries are written.
// BOTH = true (one set): (col = i, count) goes to row j as well; BOTH = false (two sets): the i side only, j numbers the other set.
template <typename Src, typename V, bool SCATTER, bool BOTH>
__global__ __launch_bounds__(LSH_THREADS) void k_lsh_knn_entries(Src src, int64_t slots, const V *__restrict__ count,
                                                                 const uint8_t *__restrict__ keep, unsigned long long *__restrict__ at,
                                                                 int32_t *__restrict__ out_col, V *__restrict__ out_count) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (LSH_THREADS / 64), chunks = (slots + 63) >> 6;
  for (int64_t c = (int64_t)blockIdx.x * (LSH_THREADS / 64) + (threadIdx.x >> 6); c < chunks; c += nwaves) {
    const int64_t s = c * 64 + lane;
    const bool kp = s < slots && keep[s] != 0;
    unsigned long long todo = __ballot(kp);
    if (!todo) continue;                          // wave-uniform
    int i = -1, j = -1, t = 0;
    V cv = 0;
    if (kp) {
      src.get(s, i, j, t);
      cv = count[s];
      if (BOTH) {
        const unsigned long long pos = atomicAdd(&at[j], 1ull);
        if (SCATTER) { out_col[pos] = i; out_count[pos] = cv; }
      }
    }
    while (todo) {                                // one round per distinct i of the chunk
      const int leader = __ffsll((long long)todo) - 1;
      const int li = __shfl(i, leader);
      const unsigned long long same = __ballot(kp && i == li);
      unsigned long long base = 0;
      if (lane == leader) base = atomicAdd(&at[li], (unsigned long long)__popcll(same));
      if (SCATTER) {
        base = lsh_shfl64(base, leader);
        if (kp && i == li) {
          const unsigned long long pos = base + (unsigned long long)__popcll(same & ((1ull << lane) - 1));
          out_col[pos] = j;
          out_count[pos] = cv;
        }
      }
      todo &= ~same;
    }
  }
}

// *out += the list entries the selection writes: the sum of min(degree, top)
__global__ __launch_bounds__(LSH_THREADS) void k_lsh_knn_written(const long long *__restrict__ ptr, int64_t n, int64_t nnz, int top,
                                                                 unsigned long long *__restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned long long sum = 0;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
    int64_t b, e;
    lsh_knn_segment(ptr, r, nnz, b, e);
    sum += (unsigned long long)min(e - b, (int64_t)top);
  }
  for (int o = 32; o > 0; o >>= 1) sum += lsh_shfl_xor64(sum, o);
  if ((threadIdx.x & 63) == 0 && sum) atomicAdd(out, sum);
}

// entry t of row r: the word's column and count, or the padding -1 / 0
template <typename K>
__device__ __forceinline__ void lsh_knn_put(unsigned long long word, bool real, int32_t *__restrict__ idx, K *__restrict__ key) {
  *idx = real ? (int32_t)(uint32_t)(word & 0xFFFFFFFFull) : -1;
  *key = real ? (K)(KnnKey<K>::MAX - (word >> 32)) : (K)0;
}

template <typename K>
__global__ __launch_bounds__(LSH_THREADS) void k_lsh_knn_select_short(const long long *__restrict__ ptr, int64_t nnz, const int32_t *__restrict__ col,
                                                                      const K *__restrict__ count, int64_t n, int top, int32_t *__restrict__ idx,
                                                                      int64_t ld_idx, K *__restrict__ key, int64_t ld_key) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (LSH_THREADS / 64);
  for (int64_t r = (int64_t)blockIdx.x * (LSH_THREADS / 64) + (threadIdx.x >> 6); r < n; r += nwaves) {
    int64_t b, e;
    lsh_knn_segment(ptr, r, nnz, b, e);
    const int deg = (int)min(e - b, (int64_t)(LSH_KNN_WAVE_MAX + 1));
    if (deg > LSH_KNN_WAVE_MAX) continue;         // wave-uniform: the long kernel's row
    unsigned long long word = lane < deg ? lsh_knn_word(col[b + lane], count[b + lane]) : ~0ull;
    for (int k = 2; (k >> 1) < deg; k <<= 1)      // bitonic, ascending; the lanes behind the row hold the largest word
      for (int j = k >> 1; j > 0; j >>= 1) {
        const unsigned long long other = lsh_shfl_xor64(word, j);
        const bool take_min = ((lane & j) == 0) == ((lane & k) == 0);
        word = take_min ? min(word, other) : max(word, other);
      }
    const int real = min(deg, top);
    for (int t = lane; t < top; t += 64) lsh_knn_put(word, t < real, idx + r * ld_idx + t, key + r * ld_key + t);
  }
}

template <typename K>
__global__ __launch_bounds__(LSH_THREADS) void k_lsh_knn_select_long(const long long *__restrict__ ptr, int64_t nnz, const int32_t *__restrict__ col,
                                                                     const K *__restrict__ count, int64_t n, int top, int32_t *__restrict__ idx,
                                                                     int64_t ld_idx, K *__restrict__ key, int64_t ld_key) {
  constexpr int TOP_DIGIT = KnnKey<K>::DIGITS - 1;
  __shared__ unsigned long long buf[LSH_KNN_LDS_WORDS];
  __shared__ unsigned int hist[256];
  __shared__ unsigned int wtot[LSH_THREADS / 64];
  __shared__ int long_rows[LSH_KNN_TILE];
  __shared__ unsigned int ctl[5];                 // long rows of the tile; the digit's bin, the entries below it, those in it; the compaction cursor
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t tiles = (n + LSH_KNN_TILE - 1) / LSH_KNN_TILE;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    if (tid == 0) ctl[0] = 0;
    __syncthreads();
    {
      const int64_t r = tile * LSH_KNN_TILE + tid;
      if (r < n) {
        int64_t b, e;
        lsh_knn_segment(ptr, r, nnz, b, e);
        if (e - b > LSH_KNN_WAVE_MAX) long_rows[atomicAdd(&ctl[0], 1u)] = tid;
      }
    }
    __syncthreads();
    const int n_long = (int)ctl[0];
    for (int q = 0; q < n_long; ++q) {
      const int64_t r = tile * LSH_KNN_TILE + long_rows[q];
      int64_t b, e;
      lsh_knn_segment(ptr, r, nnz, b, e);
      const int64_t deg = e - b;
      int have;
      if (deg <= LSH_KNN_LDS_WORDS) {
        for (int64_t p = tid; p < deg; p += LSH_THREADS) buf[p] = lsh_knn_word(col[b + p], count[b + p]);
        have = (int)deg;
      } else {                                    // top <= DA_TOPK_MAX < deg: the top-th smallest word exists
        unsigned long long prefix = 0, T = 0;
        unsigned int need = (unsigned int)top;
        for (int d = TOP_DIGIT; d >= 0; --d) {
          const int shift = 8 * d;
          hist[tid] = 0;
          __syncthreads();
          for (int64_t p0 = 0; p0 < deg; p0 += LSH_THREADS) {
            const int64_t p = p0 + tid;
            unsigned long long w = 0;
            bool m = false;
            if (p < deg) {
              w = lsh_knn_word(col[b + p], count[b + p]);
              m = d == TOP_DIGIT || ((w >> shift) >> 8) == ((prefix >> shift) >> 8);   // two shifts: shift + 8 is 64 at the uint32 key's top digit
            }
            const int digit = (int)((w >> shift) & 255);
            const unsigned long long mm = __ballot(m);
            if (!mm) continue;                    // wave-uniform
            const int d0 = __shfl(digit, __ffsll((long long)mm) - 1);
            if (__ballot(m && digit == d0) == mm) {   // one digit in the whole wave (equal counts, say): one add
              if (lane == __ffsll((long long)mm) - 1) atomicAdd(&hist[d0], (unsigned int)__popcll(mm));
            } else if (m) {
              atomicAdd(&hist[digit], 1u);
            }
          }
          __syncthreads();
          const unsigned int h = hist[tid];
          unsigned int all;
          const unsigned int excl = wg_excl_scan<LSH_THREADS / 64>(h, wtot, &all);
          if (h && excl < need && need <= excl + h) { ctl[1] = (unsigned int)tid; ctl[2] = excl; ctl[3] = h; }   // one bin holds the need-th entry
          __syncthreads();
          const unsigned int bin = ctl[1], below = ctl[2], inbin = ctl[3];
          prefix |= (unsigned long long)bin << shift;
          T = prefix | ((1ull << shift) - 1);
          if (below + inbin == need) break;       // everything up to this bin is the selection: the digits behind need no look
          need -= below;
        }
        if (tid == 0) ctl[4] = 0;
        __syncthreads();
        for (int64_t p = tid; p < deg; p += LSH_THREADS) {
          const unsigned long long w = lsh_knn_word(col[b + p], count[b + p]);
          if (w <= T) {
            const unsigned int at = atomicAdd(&ctl[4], 1u);
            if (at < (unsigned int)DA_TOPK_MAX) buf[at] = w;   // exactly `top` words when the columns are distinct, as the contract says
          }
        }
        __syncthreads();
        have = (int)min(ctl[4], (unsigned int)DA_TOPK_MAX);
      }
      int p2 = 2;
      while (p2 < have) p2 <<= 1;
      for (int a = have + tid; a < p2; a += LSH_THREADS) buf[a] = ~0ull;
      __syncthreads();
      wg_bitonic_sort<false, LSH_THREADS>(buf, p2);
      const int real = min(have, top);
      for (int t = tid; t < top; t += LSH_THREADS) lsh_knn_put(t < real ? buf[t] : 0ull, t < real, idx + r * ld_idx + t, key + r * ld_key + t);
      __syncthreads();                            // the buffer and the control words are the next row's
    }
  }
}

template <typename K>
int knn_select(const int64_t *d_ptr, int64_t nnz, const int32_t *d_col, const K *d_count, int64_t n, int top, int32_t *d_idx, int64_t ld_idx, K *d_key,
               int64_t ld_key, hipStream_t stream) {
  if (n <= 0) return DA_OK;
  const long long *ptr = reinterpret_cast<const long long *>(d_ptr);
  hipLaunchKernelGGL(k_lsh_knn_select_short<K>, dim3(lsh_grid(n * 64)), dim3(LSH_THREADS), 0, stream, ptr, nnz, d_col, d_count, n, top, d_idx, ld_idx, d_key,
                     ld_key);
  DA_HIP_TRY(hipGetLastError());
  const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(n, LSH_KNN_TILE), 256 * 8);
  hipLaunchKernelGGL(k_lsh_knn_select_long<K>, dim3(grid), dim3(LSH_THREADS), 0, stream, ptr, nnz, d_col, d_count, n, top, d_idx, ld_idx, d_key, ld_key);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}
}  // namespace

int launch_lsh_knn_select(const int64_t *d_ptr, int64_t nnz, const int32_t *d_col, const uint16_t *d_count, int64_t n, int top, int32_t *d_idx,
                          int64_t ld_idx, uint16_t *d_key, int64_t ld_key, hipStream_t stream) {
  return knn_select<uint16_t>(d_ptr, nnz, d_col, d_count, n, top, d_idx, ld_idx, d_key, ld_key, stream);
}
int launch_nw_knn_select(const int64_t *d_ptr, int64_t nnz, const int32_t *d_col, const uint32_t *d_rank_key, int64_t n, int top, int32_t *d_idx,
                         int64_t ld_idx, uint32_t *d_key, int64_t ld_key, hipStream_t stream) {
  return knn_select<uint32_t>(d_ptr, nnz, d_col, d_rank_key, n, top, d_idx, ld_idx, d_key, ld_key, stream);
}

// scratch of the scan over n + 1 degrees
size_t lsh_knn_scan_bytes(int64_t n) { return up256(scan_i64_bytes(n + 1)) + 256; }

// *d_written += the sum of min(degree, top) over the n rows of d_ptr
int launch_lsh_knn_written(const int64_t *d_ptr, int64_t n, int64_t nnz, int top, uint64_t *d_written, hipStream_t stream) {
  hipLaunchKernelGGL(k_lsh_knn_written, dim3(lsh_grid(n)), dim3(LSH_THREADS), 0, stream, reinterpret_cast<const long long *>(d_ptr), n, nnz, top,
                     reinterpret_cast<unsigned long long *>(d_written));
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

// Steps 5 and 6 on the verdicts of launch_lsh_verify_enumerated: d_ptr[rows_a + 1] = the row pointers of the entries (both: 2 per kept
// slot, the rows of one set; otherwise 1, the rows of x), d_col / d_cnt their columns and counts; d_cursor (rows_a + 1 words) is scratch,
// d_temp: lsh_knn_scan_bytes(rows_a).  *d_written (zeroed here) = the sum of min(degree, top).
namespace {
// the two passes around the scan; pass(tag) launches k_lsh_knn_entries with SCATTER = tag's value on d_cursor
template <typename Pass>
int knn_entries(int64_t rows_a, bool any, int64_t entries, int top, int64_t *d_cursor, int64_t *d_ptr, uint64_t *d_written, void *d_temp,
                size_t temp_bytes, hipStream_t stream, Pass pass) {
  DA_HIP_TRY(hipMemsetAsync(d_cursor, 0, (size_t)(rows_a + 1) * 8, stream));
  DA_HIP_TRY(hipMemsetAsync(d_written, 0, 8, stream));
  if (any) {
    pass(std::false_type());
    DA_HIP_TRY(hipGetLastError());
  }
  size_t tb = temp_bytes;
  DA_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_temp, tb, reinterpret_cast<const long long *>(d_cursor), reinterpret_cast<long long *>(d_ptr),
                                              (int)(rows_a + 1), stream));
  if (any) {
    DA_HIP_TRY(hipMemcpyAsync(d_cursor, d_ptr, (size_t)(rows_a + 1) * 8, hipMemcpyDeviceToDevice, stream));
    pass(std::true_type());
    DA_HIP_TRY(hipGetLastError());
  }
  return launch_lsh_knn_written(d_ptr, rows_a, entries, top, d_written, stream);
}
}  // namespace

int launch_lsh_knn_entries(const LshSlots &slots, int64_t rows_a, bool both, int64_t incidences, const uint16_t *d_count, const uint8_t *d_keep,
                           int64_t entries, int top, int64_t *d_cursor, int64_t *d_ptr, int32_t *d_col, uint16_t *d_cnt, uint64_t *d_written, void *d_temp,
                           size_t temp_bytes, hipStream_t stream) {
  unsigned long long *cursor = reinterpret_cast<unsigned long long *>(d_cursor);
  const unsigned grid = lsh_grid(ceil_div(incidences, 64) * 64);
  return knn_entries(rows_a, incidences > 0 && entries > 0, entries, top, d_cursor, d_ptr, d_written, d_temp, temp_bytes, stream, [&](auto scatter) {
    constexpr bool SCATTER = decltype(scatter)::value;
    with_source(slots, [&](auto src) {
      const auto kernel = both ? k_lsh_knn_entries<decltype(src), uint16_t, SCATTER, true> : k_lsh_knn_entries<decltype(src), uint16_t, SCATTER, false>;
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(LSH_THREADS), 0, stream, src, incidences, d_count, d_keep, cursor, d_col, d_cnt);
    });
  });
}

// The same on an UNPACKED candidate list with a uint32 payload (the NW lists: d_i / d_j of k_nwl_split, the value ranks and keep bytes of
// k_nwl_rank_keys): entries = the kept pairs, twice with both.  A kept pair has 0 <= i < rows_a and, with both, 0 <= j < rows_a.
int launch_nw_knn_entries(const int32_t *d_i, const int32_t *d_j, int64_t pairs, const uint32_t *d_rank_key, const uint8_t *d_keep, int64_t rows_a,
                          bool both, int64_t entries, int top, int64_t *d_cursor, int64_t *d_ptr, int32_t *d_col, uint32_t *d_val, uint64_t *d_written,
                          void *d_temp, size_t temp_bytes, hipStream_t stream) {
  unsigned long long *cursor = reinterpret_cast<unsigned long long *>(d_cursor);
  const unsigned grid = lsh_grid(ceil_div(pairs, 64) * 64);
  const LshListed src{d_i, d_j, d_i};             // the band is not read back: any readable array of `pairs` words
  return knn_entries(rows_a, pairs > 0 && entries > 0, entries, top, d_cursor, d_ptr, d_written, d_temp, temp_bytes, stream, [&](auto scatter) {
    constexpr bool SCATTER = decltype(scatter)::value;
    const auto kernel = both ? k_lsh_knn_entries<LshListed, uint32_t, SCATTER, true> : k_lsh_knn_entries<LshListed, uint32_t, SCATTER, false>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(LSH_THREADS), 0, stream, src, pairs, d_rank_key, d_keep, cursor, d_col, d_val);
  });
}

}  // namespace da
