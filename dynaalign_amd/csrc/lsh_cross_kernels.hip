// lsh_cross_kernels.hip -- MinHash LSH banding for two sets: a query batch x (m sequences) against a resident set y (n sequences) whose
// buckets are kept as an INDEX, so that a query costs a lookup and the compare of the pairs that share a bucket, never a sort of y.
// Bands, rows, cand(i, j), the count c and the first-agreeing-band rule mean what they mean in lsh_kernels.hip; the per-pair decision
// (lsh_pair_decide) and the band key (lsh_band_key) are the same functions (lsh_common.hpp).
//
//   index  the band keys of sig_y (launch_lsh_band_keys), one stable radix sort of (key, id) -- equal keys keep ids ascending -- and
//          k_lsh_index_tables: band_start[t] = the first element of band t, the number of runs and the longest one.  Layout: dynaalign.h.
//   1. k_lsh_probe: element q = i * bands + t of x computes its key and finds the run of that key inside its band's segment of the index
//      (a lower and an upper bound): lo[q], len[q]; len is 0 when the key is absent.  Consecutive lanes take consecutive bands of ONE row
//      (the walk of k_lsh_band_keys): the row is read in one stretch and lo / len are written coalesced; the searches of a wave then go
//      to `bands` different segments.  The exclusive sum of len numbers the (pair, band) incidences; its total is read back and checked
//      against the caller's cap before any pair is compared.
//   2. k_lsh_cross_verify: a wave takes 64 incidence slots; a lane finds its slot's q by a binary search of the exclusive sum, i = q /
//      bands, t = q % bands, j = ids[lo[q] + s - off[q]]; then the wave decides the 64 pairs in turn, row i of sig_x against row j of
//      sig_y.  Kept: the pair's first agreeing band only, and c >= c_min.  The same kernel runs on listed triples.
//   3. edges: the kept counts per chunk, their scan, k_lsh_cross_emit (i << 32 | j and the count into final slots, no output atomic), one
//      radix sort over 32 + bits(m) bits, launch_lsh_split.  There is no diagonal: i and j number different sets.
//   4. lists: k_lsh_cross_knn_entries counts and then scatters (col = j, count) into row i's segment -- the x rows only, one atomic per
//      distinct i of a chunk (the slots of one x row are consecutive) -- and launch_lsh_knn_select of lsh_kernels.hip takes each row's top.
#include "lsh_common.hpp"

namespace da {
namespace {

constexpr uint32_t LSH_INDEX_MAGIC = 0x4C534831u;   // "LSH1"
// meta words of the index
enum { IX_MAGIC = 0, IX_N = 1, IX_BANDS = 2, IX_ROWS = 3, IX_RUNS = 4, IX_LONGEST = 5, IX_WORDS = 8 };

struct IndexLayout {
  size_t meta, band_start, keys, ids, bytes;
  IndexLayout(int64_t total, int bands) {
    size_t at = 0;
    auto take = [&](size_t b) { const size_t o = at; at += up256(b); return o; };
    meta = take(IX_WORDS * 4);
    band_start = take(((size_t)bands + 1) * 4);
    keys = take((size_t)total * 8);
    ids = take((size_t)total * 4);
    bytes = at + 256;
  }
};

// the first p in [lo, hi) with keys[p] >= key (hi when there is none)
__device__ __forceinline__ uint32_t lsh_lower_bound(const unsigned long long *__restrict__ keys, uint32_t lo, uint32_t hi, unsigned long long key) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// On the sorted keys: band_start[t] for t = 0 .. bands (band_start[bands] = total); every last element of a run finds its run's first one
// (a lower bound in front of it), which gives the number of runs and the longest; thread 0 signs the index.
__global__ __launch_bounds__(LSH_THREADS) void k_lsh_index_tables(const unsigned long long *__restrict__ keys, uint32_t total, uint32_t n, int bands,
                                                                  int rows, uint32_t *__restrict__ band_start, uint32_t *__restrict__ meta) {
  const uint32_t stride = gridDim.x * blockDim.x, first = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t items = max(total, (uint32_t)bands + 1);
  uint32_t runs = 0, longest = 0;
  for (uint32_t p = first; p < items; p += stride) {
    if (p <= (uint32_t)bands) band_start[p] = lsh_lower_bound(keys, 0, total, (unsigned long long)p << LSH_BAND_SHIFT);
    if (p < total && (p == total - 1 || keys[p + 1] != keys[p])) {
      ++runs;
      longest = max(longest, p + 1 - lsh_lower_bound(keys, 0, p, keys[p]));
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    runs += (uint32_t)__shfl_down((int)runs, o);
    longest = max(longest, (uint32_t)__shfl_down((int)longest, o));
  }
  if ((threadIdx.x & 63) == 0 && runs) {
    atomicAdd(&meta[IX_RUNS], runs);
    atomicMax(&meta[IX_LONGEST], longest);
  }
  if (first == 0) { meta[IX_MAGIC] = LSH_INDEX_MAGIC; meta[IX_N] = n; meta[IX_BANDS] = (uint32_t)bands; meta[IX_ROWS] = (uint32_t)rows; }
}

// Element q = i * bands + t of x: lo[q] = the first element of the index whose key is x's key of band t, len = how many there are.  The
// length goes to cnt[q] (int64, cnt[elements] = 0, for the exclusive sum) and / or len32[q]; either may be NULL.  stats[0] = the longest
// probed run.  An index that was not built for (n, bands, rows) is not read: every length is 0 and stats[1] = 1.
__global__ __launch_bounds__(LSH_THREADS) void k_lsh_probe(const uint32_t *__restrict__ meta, const uint32_t *__restrict__ band_start,
                                                           const unsigned long long *__restrict__ keys, uint32_t n, const uint32_t *__restrict__ sig_x,
                                                           int64_t ld_x, int64_t elements, int bands, int rows, uint32_t *__restrict__ lo,
                                                           long long *__restrict__ cnt, int32_t *__restrict__ len32, uint32_t *__restrict__ stats) {
  const bool ok = meta[IX_MAGIC] == LSH_INDEX_MAGIC && meta[IX_N] == n && meta[IX_BANDS] == (uint32_t)bands && meta[IX_ROWS] == (uint32_t)rows;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  uint32_t longest = 0;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q <= elements; q += stride) {
    if (q == elements) {
      if (cnt) cnt[q] = 0;
      continue;
    }
    uint32_t first = 0, len = 0;
    if (ok) {
      const int64_t i = q / bands;
      const int t = (int)(q - i * bands);
      const unsigned long long key = lsh_band_key(sig_x + i * ld_x + (int64_t)t * rows, rows, t);
      const uint32_t e = band_start[t + 1];
      first = lsh_lower_bound(keys, band_start[t], e, key);
      uint32_t a = first, b = e;                   // the first element behind `first` whose key is larger
      while (a < b) {
        const uint32_t mid = a + ((b - a) >> 1);
        if (keys[mid] <= key) a = mid + 1; else b = mid;
      }
      len = a - first;
    }
    lo[q] = first;
    if (cnt) cnt[q] = (long long)len;
    if (len32) len32[q] = (int32_t)len;
    longest = max(longest, len);
  }
  for (int o = 32; o > 0; o >>= 1) longest = max(longest, (uint32_t)__shfl_down((int)longest, o));
  if ((threadIdx.x & 63) == 0 && longest) atomicMax(&stats[0], longest);
  if (!ok && blockIdx.x == 0 && threadIdx.x == 0) stats[1] = 1;
}

// ---- where the triples of the verify kernel come from: lane-level get(slot) ----------------------------------------------------------------
struct LshCrossListed {
  const int32_t *__restrict__ i, *__restrict__ j, *__restrict__ band;
  __device__ __forceinline__ void get(int64_t s, int &pi, int &pj, int &pt) const { pi = i[s]; pj = j[s]; pt = band[s]; }
};
// slot s of the exclusive sum off[0 .. elements] of the probed lengths: the element q with off[q] <= s < off[q + 1] (the LAST q with
// off[q] <= s: the elements of length 0 behind it share its successor's offset) and member s - off[q] of its run
struct LshCrossEnumerated {
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
LshCrossEnumerated enumerated(const LshCrossSlots &s) {
  return LshCrossEnumerated{reinterpret_cast<const long long *>(s.off), s.lo, s.ids, s.elements, s.bands};
}

// out_count[s] = the pair's count, out_keep[s] = 1 when the triple survives.  A triple with i outside [0, m), j outside [0, n) or a band
// outside [0, bands) reads nothing and gets 0 / 0.  chunk_kept[c] (if given) = kept triples of slots [64 c, 64 c + 64); *distinct (if
// given) += the triples that are their pair's first agreeing band, whatever their count.
template <typename Src>
__global__ __launch_bounds__(LSH_THREADS) void k_lsh_cross_verify(const uint32_t *__restrict__ sig_x, int64_t m, int64_t ld_x,
                                                                  const uint32_t *__restrict__ sig_y, int64_t n, int64_t ld_y, int n_hash, int bands,
                                                                  int rows, uint32_t c_min, Src src, int64_t slots, uint16_t *__restrict__ out_count,
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
      valid = i >= 0 && i < m && j >= 0 && j < n && t >= 0 && t < bands;
    }
    unsigned long long todo = __ballot(valid);
    uint32_t my_count = 0;
    bool my_first = false;
    while (todo) {
      const int b = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int bi = __shfl(i, b), bj = __shfl(j, b), bt = __shfl(t, b);
      const LshVerdict v = lsh_pair_decide(sig_x + (int64_t)bi * ld_x, sig_y + (int64_t)bj * ld_y, n_hash, bands * rows, rows, bt);
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

// the kept slots of chunk c, in slot order, at edge slots chunk_off[c] ...: key = i << 32 | j, value = the count
__global__ __launch_bounds__(LSH_THREADS) void k_lsh_cross_emit(LshCrossEnumerated src, int64_t slots, const uint16_t *__restrict__ count,
                                                                const uint8_t *__restrict__ keep, const long long *__restrict__ chunk_off,
                                                                unsigned long long *__restrict__ out_key, uint16_t *__restrict__ out_val) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (LSH_THREADS / 64), chunks = (slots + 63) >> 6;
  for (int64_t c = (int64_t)blockIdx.x * (LSH_THREADS / 64) + (threadIdx.x >> 6); c < chunks; c += nwaves) {
    const int64_t s = c * 64 + lane;
    const bool kp = s < slots && keep[s] != 0;
    const unsigned long long kept = __ballot(kp);
    if (!kp) continue;
    int i, j, t;
    src.get(s, i, j, t);
    const int64_t slot = chunk_off[c] + __popcll(kept & ((1ull << lane) - 1));
    out_key[slot] = ((unsigned long long)(uint32_t)i << 32) | (uint32_t)j;
    out_val[slot] = count[s];
  }
}

// The x side only.  SCATTER = false: at[] are the degrees.  SCATTER = true: at[] are the cursors (they start as the row pointers) and
// (col = j, count) is written.  One atomic per distinct i of a chunk: the slots of one x row are consecutive, so a chunk holds few of them.
template <bool SCATTER>
__global__ __launch_bounds__(LSH_THREADS) void k_lsh_cross_knn_entries(LshCrossEnumerated src, int64_t slots, const uint16_t *__restrict__ count,
                                                                       const uint8_t *__restrict__ keep, unsigned long long *__restrict__ at,
                                                                       int32_t *__restrict__ out_col, uint16_t *__restrict__ out_count) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (LSH_THREADS / 64), chunks = (slots + 63) >> 6;
  for (int64_t c = (int64_t)blockIdx.x * (LSH_THREADS / 64) + (threadIdx.x >> 6); c < chunks; c += nwaves) {
    const int64_t s = c * 64 + lane;
    const bool kp = s < slots && keep[s] != 0;
    unsigned long long todo = __ballot(kp);
    if (!todo) continue;                          // wave-uniform
    int i = -1, j = -1, t = 0;
    uint16_t cv = 0;
    if (kp) {
      src.get(s, i, j, t);
      cv = count[s];
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

// the probe workspace of `elements` = m * bands elements, cut into its arrays
struct ProbeLayout {
  size_t lo, cnt, off, stats, temp, temp_bytes, bytes;
  explicit ProbeLayout(int64_t elements) {
    const size_t t = (size_t)elements;
    size_t at = 0;
    auto take = [&](size_t b) { const size_t o = at; at += up256(b); return o; };
    lo = take(t * 4);
    cnt = take((t + 1) * 8);
    off = take((t + 1) * 8);
    stats = take(16);
    temp_bytes = scan_i64_bytes(elements + 1);
    temp = take(temp_bytes);
    bytes = at + 256;
  }
};

bool elements_ok(int64_t n, int bands) { return n > 0 && bands > 0 && n <= 0x7ffffff0LL && n * (int64_t)bands <= LSH_MAX_ELEMENTS; }

int launch_probe(const LshIndexView &ix, int64_t n, const uint32_t *d_sig_x, int64_t m, int64_t ld_x, int bands, int rows, uint32_t *d_lo,
                 long long *d_cnt, int32_t *d_len, uint32_t *d_stats, hipStream_t stream) {
  const int64_t elements = m * bands;
  DA_HIP_TRY(hipMemsetAsync(d_stats, 0, 16, stream));
  hipLaunchKernelGGL(k_lsh_probe, dim3(lsh_grid(elements + 1)), dim3(LSH_THREADS), 0, stream, ix.meta, ix.band_start,
                     reinterpret_cast<const unsigned long long *>(ix.keys), (uint32_t)n, d_sig_x, ld_x, elements, bands, rows, d_lo, d_cnt, d_len, d_stats);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

}  // namespace

size_t lsh_index_bytes(int64_t n, int bands) {
  if (bands <= 0 || n < 0 || (n > 0 && !elements_ok(n, bands))) return 256;
  return IndexLayout(n * bands, bands).bytes;
}

LshIndexView lsh_index_view(const void *d_index, int64_t n, int bands) {
  const IndexLayout L(n * bands, bands);
  void *base = align256(const_cast<void *>(d_index));
  return LshIndexView{at_bytes<const uint32_t>(base, L.meta), at_bytes<const uint32_t>(base, L.band_start), at_bytes<const uint64_t>(base, L.keys),
                      at_bytes<const int32_t>(base, L.ids)};
}

// unsorted keys and ids, and the sort's scratch
size_t lsh_index_build_scratch_bytes(int64_t n, int bands) {
  const size_t t = (size_t)(n * bands);
  return up256(t * 8) + up256(t * 4) + up256(sort_u64_i32_bytes(n * bands)) + 256;
}

int lsh_index_build(const uint32_t *d_sig, int64_t n, int64_t ld_sig, int bands, int rows, void *d_index, void *d_scratch, hipStream_t stream) {
  const int64_t total = n * bands;
  const LshIndexView ix = lsh_index_view(d_index, n, bands);
  uint32_t *meta = const_cast<uint32_t *>(ix.meta);
  unsigned long long *keys = reinterpret_cast<unsigned long long *>(const_cast<uint64_t *>(ix.keys));
  d_scratch = align256(d_scratch);
  unsigned long long *keys_in = at_bytes<unsigned long long>(d_scratch, 0);
  int32_t *ids_in = at_bytes<int32_t>(d_scratch, up256((size_t)total * 8));
  void *temp = at_bytes<char>(d_scratch, up256((size_t)total * 8) + up256((size_t)total * 4));
  size_t tb = sort_u64_i32_bytes(total);
  int rc;
  DA_HIP_TRY(hipMemsetAsync(meta, 0, IX_WORDS * 4, stream));
  if ((rc = launch_lsh_band_keys(d_sig, n, ld_sig, bands, rows, reinterpret_cast<uint64_t *>(keys_in), ids_in, stream)) != DA_OK) return rc;
  DA_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(temp, tb, keys_in, keys, ids_in, const_cast<int32_t *>(ix.ids), (int)total, 0,
                                                LSH_BAND_SHIFT + bits_for(bands), stream));
  hipLaunchKernelGGL(k_lsh_index_tables, dim3(lsh_grid(std::max<int64_t>(total, bands + 1))), dim3(LSH_THREADS), 0, stream, keys, (uint32_t)total,
                     (uint32_t)n, bands, rows, const_cast<uint32_t *>(ix.band_start), meta);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

size_t lsh_cross_workspace_bytes(int64_t m, int bands) {
  if (!elements_ok(m, bands)) return 256;
  return ProbeLayout(m * bands).bytes;
}

int lsh_index_probe_listed(const void *d_index, int64_t n, const uint32_t *d_sig_x, int64_t m, int64_t ld_x, int bands, int rows, int32_t *d_lo,
                           int32_t *d_len, uint32_t *d_stats, int *mismatch_host, hipStream_t stream) {
  int rc;
  if ((rc = launch_probe(lsh_index_view(d_index, n, bands), n, d_sig_x, m, ld_x, bands, rows, reinterpret_cast<uint32_t *>(d_lo), nullptr, d_len, d_stats,
                         stream)) != DA_OK) return rc;
  uint32_t stats[2] = {0, 0};
  DA_HIP_TRY(hipMemcpyAsync(stats, d_stats, 8, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipStreamSynchronize(stream));
  *mismatch_host = (int)stats[1];
  return DA_OK;
}

int lsh_cross_probe(const void *d_index, int64_t n, const uint32_t *d_sig_x, int64_t m, int64_t ld_x, int bands, int rows, void *d_work, size_t work_bytes,
                    LshCrossSlots *slots_out, uint32_t stats_host[3], int64_t *incidences_host, hipStream_t stream) {
  const int64_t elements = m * bands;
  const ProbeLayout L(elements);
  if (!d_work || work_bytes < L.bytes) return fail(DA_ERR_BAD_ARG, "lsh: workspace too small (%zu bytes, %zu needed)", work_bytes, L.bytes);
  d_work = align256(d_work);                      // the arrays start on 256 bytes whatever the caller's pointer
  const LshIndexView ix = lsh_index_view(d_index, n, bands);
  uint32_t *lo = at_bytes<uint32_t>(d_work, L.lo), *stats = at_bytes<uint32_t>(d_work, L.stats);
  long long *cnt = at_bytes<long long>(d_work, L.cnt), *off = at_bytes<long long>(d_work, L.off);
  int rc;
  if ((rc = launch_probe(ix, n, d_sig_x, m, ld_x, bands, rows, lo, cnt, nullptr, stats, stream)) != DA_OK) return rc;
  size_t tb = L.temp_bytes;
  DA_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(at_bytes<char>(d_work, L.temp), tb, cnt, off, (int)(elements + 1), stream));
  long long inc = 0;
  uint32_t probed[2] = {0, 0}, runs = 0;
  DA_HIP_TRY(hipMemcpyAsync(&inc, off + elements, 8, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipMemcpyAsync(probed, stats, 8, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipMemcpyAsync(&runs, ix.meta + IX_RUNS, 4, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipStreamSynchronize(stream));
  stats_host[0] = probed[0]; stats_host[1] = runs; stats_host[2] = probed[1];
  *incidences_host = (int64_t)inc;
  *slots_out = LshCrossSlots{reinterpret_cast<const int64_t *>(off), lo, ix.ids, elements, bands};
  return DA_OK;
}

int launch_lsh_cross_verify_listed(const uint32_t *d_sig_x, int64_t m, int64_t ld_x, const uint32_t *d_sig_y, int64_t n, int64_t ld_y, int n_hash, int bands,
                                   int rows, uint32_t c_min, const int32_t *d_i, const int32_t *d_j, const int32_t *d_band, int64_t triples,
                                   uint16_t *d_count, uint8_t *d_keep, hipStream_t stream) {
  if (triples <= 0) return DA_OK;
  hipLaunchKernelGGL(k_lsh_cross_verify<LshCrossListed>, dim3(lsh_grid(ceil_div(triples, 64) * 64)), dim3(LSH_THREADS), 0, stream, d_sig_x, m, ld_x, d_sig_y,
                     n, ld_y, n_hash, bands, rows, c_min, LshCrossListed{d_i, d_j, d_band}, triples, d_count, d_keep, (long long *)nullptr,
                     (unsigned long long *)nullptr);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

// Step 2 on the enumerated incidences: verdicts into d_count / d_keep (one per incidence), kept counts per chunk of 64 into d_chunk_kept
// (chunks + 1 entries, the last one 0), their exclusive sum into d_chunk_off (d_temp: lsh_chunk_scan_bytes(incidences)); *d_distinct
// (zeroed here) counts the distinct candidate pairs.
int launch_lsh_cross_verify_enumerated(const uint32_t *d_sig_x, int64_t m, int64_t ld_x, const uint32_t *d_sig_y, int64_t n, int64_t ld_y, int n_hash,
                                       int rows, uint32_t c_min, const LshCrossSlots &slots, int64_t incidences, uint16_t *d_count, uint8_t *d_keep,
                                       int64_t *d_chunk_kept, int64_t *d_chunk_off, uint64_t *d_distinct, void *d_temp, size_t temp_bytes,
                                       hipStream_t stream) {
  const int64_t chunks = ceil_div(incidences, 64);
  DA_HIP_TRY(hipMemsetAsync(d_distinct, 0, 8, stream));
  DA_HIP_TRY(hipMemsetAsync(d_chunk_kept + chunks, 0, 8, stream));
  if (incidences > 0) {
    hipLaunchKernelGGL(k_lsh_cross_verify<LshCrossEnumerated>, dim3(lsh_grid(chunks * 64)), dim3(LSH_THREADS), 0, stream, d_sig_x, m, ld_x, d_sig_y, n, ld_y,
                       n_hash, slots.bands, rows, c_min, enumerated(slots), incidences, d_count, d_keep, reinterpret_cast<long long *>(d_chunk_kept),
                       reinterpret_cast<unsigned long long *>(d_distinct));
    DA_HIP_TRY(hipGetLastError());
  }
  size_t tb = temp_bytes;
  DA_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_temp, tb, reinterpret_cast<const long long *>(d_chunk_kept), reinterpret_cast<long long *>(d_chunk_off),
                                              (int)(chunks + 1), stream));
  return DA_OK;
}

// Step 3: the kept incidences into d_key_in / d_val_in (`edges` entries, > 0), sorted by (i, j) into d_key_out / d_val_out
// (d_temp: lsh_edge_sort_bytes(edges)).
int launch_lsh_cross_emit_sort(const LshCrossSlots &slots, int64_t m, int64_t incidences, const uint16_t *d_count, const uint8_t *d_keep,
                               const int64_t *d_chunk_off, int64_t edges, uint64_t *d_key_in, uint16_t *d_val_in, uint64_t *d_key_out,
                               uint16_t *d_val_out, void *d_temp, size_t temp_bytes, hipStream_t stream) {
  if (incidences <= 0 || edges <= 0) return DA_OK;
  unsigned long long *kin = reinterpret_cast<unsigned long long *>(d_key_in), *kout = reinterpret_cast<unsigned long long *>(d_key_out);
  hipLaunchKernelGGL(k_lsh_cross_emit, dim3(lsh_grid(ceil_div(incidences, 64) * 64)), dim3(LSH_THREADS), 0, stream, enumerated(slots), incidences, d_count,
                     d_keep, reinterpret_cast<const long long *>(d_chunk_off), kin, d_val_in);
  DA_HIP_TRY(hipGetLastError());
  size_t tb = temp_bytes;
  DA_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(d_temp, tb, kin, kout, d_val_in, d_val_out, (int)edges, 0, 32 + bits_for(m), stream));
  return DA_OK;
}

// Step 4 on the verdicts: d_ptr[m + 1] = the row pointers of the x rows' entries (one per kept slot), d_col / d_cnt their columns and
// counts; d_cursor (m + 1 words) is scratch, d_temp: lsh_knn_scan_bytes(m).  *d_written (zeroed here) = the sum of min(degree, top).
int launch_lsh_cross_knn_entries(const LshCrossSlots &slots, int64_t m, int64_t incidences, const uint16_t *d_count, const uint8_t *d_keep, int64_t entries,
                                 int top, int64_t *d_cursor, int64_t *d_ptr, int32_t *d_col, uint16_t *d_cnt, uint64_t *d_written, void *d_temp,
                                 size_t temp_bytes, hipStream_t stream) {
  unsigned long long *cursor = reinterpret_cast<unsigned long long *>(d_cursor);
  const unsigned grid = lsh_grid(ceil_div(incidences, 64) * 64);
  DA_HIP_TRY(hipMemsetAsync(d_cursor, 0, (size_t)(m + 1) * 8, stream));
  DA_HIP_TRY(hipMemsetAsync(d_written, 0, 8, stream));
  if (incidences > 0 && entries > 0) {
    hipLaunchKernelGGL(k_lsh_cross_knn_entries<false>, dim3(grid), dim3(LSH_THREADS), 0, stream, enumerated(slots), incidences, d_count, d_keep, cursor,
                       (int32_t *)nullptr, (uint16_t *)nullptr);
    DA_HIP_TRY(hipGetLastError());
  }
  size_t tb = temp_bytes;
  DA_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_temp, tb, reinterpret_cast<const long long *>(d_cursor), reinterpret_cast<long long *>(d_ptr), (int)(m + 1),
                                              stream));
  if (incidences > 0 && entries > 0) {
    DA_HIP_TRY(hipMemcpyAsync(d_cursor, d_ptr, (size_t)(m + 1) * 8, hipMemcpyDeviceToDevice, stream));
    hipLaunchKernelGGL(k_lsh_cross_knn_entries<true>, dim3(grid), dim3(LSH_THREADS), 0, stream, enumerated(slots), incidences, d_count, d_keep, cursor, d_col,
                       d_cnt);
    DA_HIP_TRY(hipGetLastError());
  }
  return launch_lsh_knn_written(d_ptr, m, entries, top, d_written, stream);
}

}  // namespace da
