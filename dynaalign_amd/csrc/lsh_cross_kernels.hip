// lsh_cross_kernels.hip -- the two-set FRONT END of MinHash LSH banding: a query batch x (m sequences) against a resident set y (n
// sequences) whose buckets are kept as an INDEX, so that a query costs a lookup and the compare of the pairs that share a bucket, never a
// sort of y.  Bands, rows, cand(i, j), the count c and the first-agreeing-band rule mean what they mean in lsh_kernels.hip, and the band
// key (lsh_band_key) is the same function (lsh_common.hpp).  This file is the index and the probe; what follows them -- verify, the edge
// list, the lists -- is the back end in lsh_kernels.hip, which takes the probe's LshSlots.
//
//   index  the band keys of sig_y (launch_lsh_band_keys), one stable radix sort of (key, id) -- equal keys keep ids ascending -- and
//          k_lsh_index_tables: band_start[t] = the first element of band t, the number of runs and the longest one.  Layout: dynaalign.h.
//   probe  k_lsh_probe: element q = i * bands + t of x computes its key and finds the run of that key inside its band's segment of the
//          index (a lower and an upper bound): lo[q], len[q]; len is 0 when the key is absent.  Consecutive lanes take consecutive bands of
//          ONE row (the walk of k_lsh_band_keys): the row is read in one stretch and lo / len are written coalesced; the searches of a wave
//          then go to `bands` different segments.  The exclusive sum of len numbers the (pair, band) incidences: slot s of element q is
//          (i = q / bands, j = ids[lo[q] + s - off[q]], band = q % bands).  The total is read back and checked against the caller's cap
//          before any pair is compared.
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
                    LshSlots *slots_out, uint32_t stats_host[3], int64_t *incidences_host, hipStream_t stream) {
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
  *slots_out = LshSlots{true, reinterpret_cast<const int64_t *>(off), ix.ids, nullptr, lo, elements, bands};
  return DA_OK;
}

}  // namespace da
