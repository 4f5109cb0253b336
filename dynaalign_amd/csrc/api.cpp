// api.cpp -- the C ABI of libdynaalign_hip.so (see include/dynaalign.h).
//
// Host-side marshalling only: argument validation with the reference's error
// order and message texts, packing, H2D/D2H, and kernel launches.  There is
// deliberately NO CPU implementation of the hot path in this library.
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <condition_variable>
#include <cstddef>
#include <map>
#include <memory>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "da_common.hpp"

namespace da { size_t destroy_cached_comms(); }   // defined with the multi-device entry points

namespace da {

const signed char *matrix_table_host(int id);
const char *matrix_name_host(int id);
int matrix_count_host();

std::string &last_error_ref() {
  static thread_local std::string msg;
  return msg;
}

int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  last_error_ref() = buf;
  return code;
}

namespace {

// Large device buffers are kept for the next call instead of going back to the driver: hipMalloc / hipFree of the
// 80 GB result buffer cost up to 3.2 s every other call on MI355X (profiles/r02_b_host_path_trace.txt) -- more than the
// 1.5 s the PCIe copy of the result takes -- and clusterbreak calls sim_fn again and again.  Per device up to MAX_PARKED
// buffers of >= 1 MiB totalling at most 30 % of the device's memory are parked (one call of the duplicate-collapsing routes uses four:
// plan, table, gathered table, plane workspace); a request takes the smallest parked buffer that fits it and is at most
// twice its size (a 300 MB request must not walk away with the 9 GB buffer the next allocation of the same call wants);
// when room is needed the smallest parked buffers go first (cheapest to allocate again).  da_release_device_memory()
// returns everything to the driver, and so does an allocation of ours that would otherwise fail.
struct BigCache {
  static constexpr size_t MIN_BYTES = (size_t)1 << 20;     // (hipFree synchronises the device: even the 10 MB plan is worth keeping)
  static constexpr int MAX_PARKED = 16;
  struct Ent { int dev; void *p; size_t bytes; };
  std::mutex m;
  std::vector<Ent> parked;
  std::vector<size_t> budget;                                   // per device: 30 % of its memory (0 = not asked yet)
  size_t budget_of(int dev) {
    if ((size_t)dev >= budget.size()) budget.resize((size_t)dev + 1, 0);
    if (!budget[(size_t)dev]) {
      size_t total_b = 0;
      const int pct = da::config().buffer_cache_pct;         // DYNAALIGN_BUFFER_CACHE_PCT: share of the device's memory that may stay parked (30)
      budget[(size_t)dev] = hipDeviceTotalMem(&total_b, dev) == hipSuccess && total_b ? total_b / 100 * (size_t)pct : (size_t)64 << 30;
      if (!budget[(size_t)dev]) budget[(size_t)dev] = 1;       // 0 % = park nothing (but do not ask again)
    }
    return budget[(size_t)dev];
  }
  void *take(int dev, size_t bytes, size_t *cap) {
    std::lock_guard<std::mutex> g(m);
    size_t best = parked.size();
    for (size_t i = 0; i < parked.size(); ++i)
      if (parked[i].dev == dev && parked[i].bytes >= bytes && parked[i].bytes / 2 <= bytes &&
          (best == parked.size() || parked[i].bytes < parked[best].bytes)) best = i;
    if (best == parked.size()) return nullptr;
    void *p = parked[best].p;
    *cap = parked[best].bytes;
    parked.erase(parked.begin() + (long)best);
    // a buffer may have been parked by an early return with kernels still in flight on some stream: nothing may still be
    // touching it when its next owner -- possibly on another stream or thread -- starts writing (the device is idle here in
    // the normal case: the call that parked it ended with a synchronisation, so this costs microseconds)
    (void)hipDeviceSynchronize();
    return p;
  }
  void park(int dev, void *p, size_t bytes) {                   // (the caller has made `dev` current)
    std::lock_guard<std::mutex> g(m);
    const size_t cap_bytes = budget_of(dev);
    if (bytes > cap_bytes) { (void)hipFree(p); return; }
    for (;;) {
      int mine = 0;
      size_t sum = 0, smallest = parked.size();
      for (size_t i = 0; i < parked.size(); ++i)
        if (parked[i].dev == dev) {
          ++mine; sum += parked[i].bytes;
          if (smallest == parked.size() || parked[i].bytes < parked[smallest].bytes) smallest = i;
        }
      if (mine < MAX_PARKED && sum + bytes <= cap_bytes) break;
      if (parked[smallest].bytes >= bytes) { (void)hipFree(p); return; }   // everything parked is bigger: the newcomer goes
      (void)hipFree(parked[smallest].p);
      parked.erase(parked.begin() + (long)smallest);
    }
    parked.push_back({dev, p, bytes});
  }
  size_t release(int dev_or_all) {
    std::lock_guard<std::mutex> g(m);
    size_t freed = 0;
    for (size_t i = 0; i < parked.size();)
      if (dev_or_all < 0 || parked[i].dev == dev_or_all) { (void)hipFree(parked[i].p); freed += parked[i].bytes; parked.erase(parked.begin() + (long)i); }
      else ++i;
    return freed;
  }
};
BigCache &big_cache() { static BigCache *c = new BigCache; return *c; }   // never destroyed: the HIP runtime may be gone at exit

// RAII device buffer
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  int dev = 0;
  ~DevBuf() { release(); }
  void release() {   // back to the cache (or freed) now
    if (!p) return;
    if (cap >= BigCache::MIN_BYTES && !da::config().no_buffer_cache) big_cache().park(dev, p, cap);
    else (void)hipFree(p);
    p = nullptr;
  }
  int alloc(size_t bytes) {
    if (bytes == 0) bytes = 16;
    (void)hipGetDevice(&dev);
    if (bytes >= BigCache::MIN_BYTES && (p = big_cache().take(dev, bytes, &cap)) != nullptr) return DA_OK;
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipErrorOutOfMemory && big_cache().release(dev) > 0) {   // parked buffers are the first thing to give back
      (void)hipGetLastError();
      e = hipMalloc(&p, bytes);
    }
    if (e != hipSuccess) {
      p = nullptr;
      return fail(e == hipErrorOutOfMemory ? DA_ERR_NOMEM : DA_ERR_HIP, "hipMalloc(%zu bytes) failed: %s", bytes,
                  hipGetErrorString(e));
    }
    cap = bytes;
    return DA_OK;
  }
  template <typename T> T *as() const { return static_cast<T *>(p); }
};

int require_device() {
  int cnt = 0;
  hipError_t e = hipGetDeviceCount(&cnt);
  if (e != hipSuccess || cnt <= 0)
    return fail(DA_ERR_NO_DEVICE,
                "no usable HIP device (%s); libdynaalign_hip has no CPU fallback",
                e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
  return DA_OK;
}

// reference src/minHash.cpp:121-131, in that order
int validate_mh(int64_t n, int k, int n_hash) {
  if (n <= 0) return fail(DA_ERR_EMPTY_INPUT, "%s", da_status_message(DA_ERR_EMPTY_INPUT));
  if (k <= 0) return fail(DA_ERR_BAD_K, "%s", da_status_message(DA_ERR_BAD_K));
  if (n_hash <= 0) return fail(DA_ERR_BAD_NHASH, "%s", da_status_message(DA_ERR_BAD_NHASH));
  return DA_OK;
}

int64_t sig_ld_for(int n_hash) { return ((int64_t)n_hash + 31) / 32 * 32; }

int check_offsets(const int64_t *offsets, int64_t n, int64_t *total, int64_t *max_len) {
  if (!offsets) return fail(DA_ERR_BAD_ARG, "offsets is NULL");
  int64_t mx = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t len = offsets[i + 1] - offsets[i];
    if (len < 0) return fail(DA_ERR_BAD_ARG, "offsets must be non-decreasing (sequence %lld)", (long long)i);
    mx = std::max(mx, len);
  }
  if (offsets[0] != 0) return fail(DA_ERR_BAD_ARG, "offsets[0] must be 0");
  *total = offsets[n];
  *max_len = mx;
  return DA_OK;
}

// Upload the packed sequences (+ optionally seeds) to the current device.
struct DeviceInput {
  DevBuf res, off, seeds;
  int upload(const uint8_t *residues, const int64_t *offsets, int64_t n, int64_t total,
             const uint32_t *seedv, int n_hash) {
    int rc;
    if ((rc = res.alloc((size_t)total)) != DA_OK) return rc;
    if ((rc = off.alloc((size_t)(n + 1) * sizeof(int64_t))) != DA_OK) return rc;
    if (total) DA_HIP_TRY(hipMemcpy(res.p, residues, (size_t)total, hipMemcpyHostToDevice));
    DA_HIP_TRY(hipMemcpy(off.p, offsets, (size_t)(n + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    if (seedv) {
      if ((rc = seeds.alloc((size_t)n_hash * sizeof(uint32_t))) != DA_OK) return rc;
      DA_HIP_TRY(hipMemcpy(seeds.p, seedv, (size_t)n_hash * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    return DA_OK;
  }
};


// Device -> caller-owned pageable host memory (the R matrix).  A plain hipMemcpy of pageable memory
// staged at ~17 GB/s (measured, profiles/r01_d_host_path.json); this ring of pinned staging buffers
// keeps the DMA engine streaming while host threads copy finished chunks into the destination.
// (hipHostRegister of the destination would pin up to 80 GB of R's heap -- not ours to pin.)
// A few persistent host threads that copy pieces of a pinned chunk into the destination (the destination's
// first-touch page faults are what they parallelise; one pool per call, not one thread per chunk).
class CopyPool {
 public:
  explicit CopyPool(int workers) {
    for (int w = 0; w < workers; ++w) th_.emplace_back([this, w]() { run(w); });
  }
  ~CopyPool() {
    { std::lock_guard<std::mutex> g(m_); stop_ = true; ++gen_; }
    cv_.notify_all();
    for (auto &t : th_) t.join();
  }
  // fn(b, e) over [0, len) split into one piece per worker + the calling thread; returns when all pieces are done
  void run_split(size_t len, const std::function<void(size_t, size_t)> &fn) {
    const size_t parts = th_.size() + 1, part = (len + parts - 1) / parts;
    { std::lock_guard<std::mutex> g(m_); fn_ = &fn; len_ = len; part_ = part; pending_ = (int)th_.size(); ++gen_; }
    cv_.notify_all();
    fn(0, std::min(part, len));
    std::unique_lock<std::mutex> g(m_);
    done_.wait(g, [this]() { return pending_ == 0; });
  }

 private:
  void run(int w) {
    uint64_t seen = 0;
    for (;;) {
      std::unique_lock<std::mutex> g(m_);
      cv_.wait(g, [&]() { return gen_ != seen; });
      seen = gen_;
      if (stop_) return;
      const std::function<void(size_t, size_t)> *fn = fn_;
      const size_t len = len_, part = part_;
      g.unlock();
      const size_t b = (size_t)(w + 1) * part;
      if (b < len) (*fn)(b, std::min(len, b + part));
      g.lock();
      if (--pending_ == 0) done_.notify_one();
    }
  }
  std::vector<std::thread> th_;
  std::mutex m_;
  std::condition_variable cv_, done_;
  uint64_t gen_ = 0;
  bool stop_ = false;
  const std::function<void(size_t, size_t)> *fn_ = nullptr;
  size_t len_ = 0, part_ = 0;
  int pending_ = 0;
};

// dst[i] = table[src[i]] with streaming stores (the destination is written once: no read-for-ownership traffic)
void widen_u16_to_f64(double *dst, const uint16_t *src, size_t b, size_t e, const double *table) {
  typedef double v2d __attribute__((ext_vector_type(2)));
  size_t i = b;
  if (i < e && (reinterpret_cast<uintptr_t>(dst + i) & 15)) { dst[i] = table[src[i]]; ++i; }
  for (; i + 2 <= e; i += 2) {
    const v2d v = {table[src[i]], table[src[i + 1]]};
    __builtin_nontemporal_store(v, reinterpret_cast<v2d *>(dst + i));
  }
  if (i < e) dst[i] = table[src[i]];
}

// Device -> caller-owned pageable host memory through the pinned ring.  With `table` the device buffer holds uint16 codes and
// the HOST widens them while copying: dst (double) [i] = table[code[i]] -- a quarter of the bytes cross PCIe (the 80 GB float64
// result of N = 100k took 1.48 s at 54 GB/s; as codes it is 20 GB), and the divide behind every table entry is the same IEEE
// operation on the host as on the device (src/minHash.cpp:174, src/pairwiseSeqAlign.cpp:311).
int d2h_pipelined(void *dst, const void *d_src, size_t bytes, const double *table = nullptr) {
  constexpr size_t CHUNK = (size_t)64 << 20, SMALL = (size_t)8 << 20;   // SMALL: codes of n <= 2048 sequences
  constexpr int RING = 4, MAX_WORKERS = 32;
  int WORKERS = table ? 16 : 8;          // host threads per chunk (first-touch page faults of the destination parallelise)
  if (da::config().d2h_threads > 0) WORKERS = std::min(MAX_WORKERS, da::config().d2h_threads);   // DYNAALIGN_D2H_THREADS
  {
    const unsigned hw = std::thread::hardware_concurrency();
    cpu_set_t cs;
    int avail = (sched_getaffinity(0, sizeof cs, &cs) == 0) ? CPU_COUNT(&cs) : (int)hw;
    if (avail > 0 && WORKERS > avail) WORKERS = avail;
  }
  if (bytes <= CHUNK && !table) {
    DA_HIP_TRY(hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
    return DA_OK;
  }
  if (bytes <= SMALL && table) {
    // small results (clusterbreak calls sim_fn on thousands of small subsets): ONE plain copy of the codes and an inline
    // widening -- no pinned ring (4 x 64 MiB of hipHostMalloc), no stream / events, no thread pool per call
    std::vector<uint16_t> codes(bytes / 2);
    DA_HIP_TRY(hipMemcpy(codes.data(), d_src, bytes, hipMemcpyDeviceToHost));
    widen_u16_to_f64(static_cast<double *>(dst), codes.data(), 0, bytes / 2, table);
    return DA_OK;
  }
  if (da::config().plain_d2h && !table) {
    DA_HIP_TRY(hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
    return DA_OK;
  }
  struct Slot { void *pin = nullptr; hipEvent_t ev = nullptr; };
  Slot ring[RING];
  hipStream_t st = nullptr;
  int rc = DA_OK;
  auto cleanup = [&]() {                 // copies still in flight on `st` must not outlive the pinned slots they write
    if (st) (void)hipStreamSynchronize(st);
    for (auto &s : ring) { if (s.pin) (void)hipHostFree(s.pin); if (s.ev) (void)hipEventDestroy(s.ev); }
    if (st) (void)hipStreamDestroy(st);
  };
  auto check = [&](hipError_t e, const char *what) {
    if (e != hipSuccess && rc == DA_OK) rc = fail(DA_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
    return e == hipSuccess;
  };
  if (!check(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "hipStreamCreate")) { cleanup(); return rc; }
  for (auto &s : ring)
    if (!check(hipHostMalloc(&s.pin, CHUNK, hipHostMallocDefault), "hipHostMalloc") ||
        !check(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming), "hipEventCreate")) { cleanup(); return rc; }
  if (!check(hipDeviceSynchronize(), "hipDeviceSynchronize")) { cleanup(); return rc; }   // the producing kernels ran on the null stream
  {
    CopyPool pool(WORKERS - 1);
    const size_t nchunk = (bytes + CHUNK - 1) / CHUNK;
    for (size_t c = 0; c < nchunk + RING - 1 && rc == DA_OK; ++c) {
      if (c < nchunk) {                  // slot c % RING was drained RING iterations ago
        const size_t off = c * CHUNK, len = std::min(CHUNK, bytes - off);
        if (!check(hipMemcpyAsync(ring[c % RING].pin, static_cast<const char *>(d_src) + off, len, hipMemcpyDeviceToHost, st), "hipMemcpyAsync") ||
            !check(hipEventRecord(ring[c % RING].ev, st), "hipEventRecord")) break;
      }
      if (c >= RING - 1) {
        const size_t done = c - (RING - 1), off = done * CHUNK, len = std::min(CHUNK, bytes - off);
        if (!check(hipEventSynchronize(ring[done % RING].ev), "hipEventSynchronize")) break;
        const char *src = static_cast<const char *>(ring[done % RING].pin);
        if (table) {
          double *d = static_cast<double *>(dst) + off / 2;                 // `bytes` counts the uint16 source
          const uint16_t *s16 = reinterpret_cast<const uint16_t *>(src);
          pool.run_split(len / 2, [=](size_t b, size_t e) { widen_u16_to_f64(d, s16, b, e, table); });
        } else {
          char *d = static_cast<char *>(dst) + off;
          pool.run_split(len, [=](size_t b, size_t e) { memcpy(d + b, src + b, e - b); });
        }
      }
    }
  }
  cleanup();
  return rc;
}

// DYNAALIGN_TRACE=1: wall-clock checkpoints of the host-pointer paths on stderr (where does T_h go?)
struct Trace {
  const bool on = da::config().trace;
  const char *what;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), last = t0;
  explicit Trace(const char *w) : what(w) {}
  void mark(const char *step) {
    if (!on) return;
    (void)hipDeviceSynchronize();
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[dynaalign] %s: %-28s %9.3f ms (total %9.3f ms)\n", what, step,
            std::chrono::duration<double, std::milli>(now - last).count(), std::chrono::duration<double, std::milli>(now - t0).count());
    last = now;
  }
};

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// How many result rows of n columns the device may hold at once (host-pointer paths): a multiple of 128, at least 128, whatever the
// number of rows there are.
size_t block_budget() {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)8 << 30;
  {
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> g(big_cache().m);       // what is parked for reuse is as good as free
    for (const auto &e : big_cache().parked) if (e.dev == dev) free_b += e.bytes;
  }
  size_t budget = free_b / 2;
  if (da::config().block_bytes) budget = (size_t)da::config().block_bytes;   // DYNAALIGN_BLOCK_BYTES
  return budget;
}
int64_t block_rows(int64_t n, size_t bytes_per_elem) {
  int64_t rows = (int64_t)(block_budget() / ((size_t)n * bytes_per_elem));
  rows = rows / 128 * 128;
  if (rows < 128) rows = 128;
  return rows;
}
// ... of a square n x n result: never more than its n rows
int64_t rows_per_block(int64_t n, size_t bytes_per_elem) { return std::min(block_rows(n, bytes_per_elem), n); }

}  // namespace
}  // namespace da

using namespace da;

// ---- run-time switches: parsed once (da_common.hpp Config) -----------------------------------------------------------------------
namespace da {
namespace {
bool env_flag(const char *name) { return getenv(name) != nullptr; }
int64_t env_i64(const char *name, int64_t dflt) { const char *e = getenv(name); return e ? atoll(e) : dflt; }
uint64_t env_u64(const char *name, uint64_t dflt) { const char *e = getenv(name); return e ? strtoull(e, nullptr, 10) : dflt; }
enum MhExpand { MH_EXPAND_DEFAULT, MH_EXPAND_ROWS, MH_EXPAND_ROWSPIPE, MH_EXPAND_PIPE, MH_EXPAND_TILES };   // Config::mh_expand
Config parse_config() {
  Config c;
  c.mh_no_dedup = env_flag("DYNAALIGN_MH_NO_DEDUP");
  c.mh_no_sparse = env_flag("DYNAALIGN_MH_NO_SPARSE");
  c.mh_no_pipe = env_flag("DYNAALIGN_MH_NO_PIPE");
  c.mh_pipe_one_stream = env_flag("DYNAALIGN_MH_PIPE_ONE_STREAM");
  c.mh_dedup_min_n = env_i64("DYNAALIGN_MH_DEDUP_MIN_N", -1);
  c.mh_dedup_max_pct = env_i64("DYNAALIGN_MH_DEDUP_MAX_PCT", -1);
  c.mh_sparse_max_pairs = std::min<uint64_t>(env_u64("DYNAALIGN_MH_SPARSE_MAX_PAIRS", 400000000ull), 0xfffffff0ull);   // (32-bit entry offsets)
  c.mh_no_hybrid = env_flag("DYNAALIGN_MH_NO_HYBRID");
  c.mh_hybrid_min_n = env_i64("DYNAALIGN_MH_HYBRID_MIN_N", -1);
  c.mh_hybrid_dedup = env_flag("DYNAALIGN_MH_HYBRID_DEDUP");
  if (const char *e = getenv("DYNAALIGN_MH_EXPAND"))
    c.mh_expand = !strcmp(e, "rows") ? MH_EXPAND_ROWS : !strcmp(e, "rowspipe") ? MH_EXPAND_ROWSPIPE : !strcmp(e, "pipe") ? MH_EXPAND_PIPE
                : !strcmp(e, "tiles") ? MH_EXPAND_TILES : MH_EXPAND_DEFAULT;
  c.mh_pipe_step = (int)std::max<int64_t>(0, env_i64("DYNAALIGN_MH_PIPE_STEP", 0));
  c.mh_pipe_wg = (int)std::max<int64_t>(0, std::min<int64_t>(4, env_i64("DYNAALIGN_MH_PIPE_WG", 0)));
  c.mh_pipe_head = (int)std::max<int64_t>(0, env_i64("DYNAALIGN_MH_PIPE_HEAD", 0));
  c.mh_expand_zones = (int)env_i64("DYNAALIGN_MH_EXPAND_ZONES", 0);
  if (const char *e = getenv("DYNAALIGN_MH_DEDUP_ORDER")) c.mh_dedup_order = !strcmp(e, "first") ? 1 : !strcmp(e, "zoned") ? 2 : 0;
  const int pb = (int)env_i64("DYNAALIGN_PLANE_BITS", 0);
  c.plane_bits = (pb == 32 || pb == 16 || pb == 15 || pb == 14 || pb == 12) ? pb : 0;
  c.k2_no_asm = env_flag("DYNAALIGN_K2_NO_ASM");
  c.k2_persist = env_flag("DYNAALIGN_K2_PERSIST");
  c.k2_wg_per_cu = (int)std::max<int64_t>(0, env_i64("DYNAALIGN_K2_WG_PER_CU", 0));
  c.nw_no_dedup = env_flag("DYNAALIGN_NW_NO_DEDUP");
  c.nw_int32 = env_flag("DYNAALIGN_NW_INT32");
  c.nw_no_prefix = env_flag("DYNAALIGN_NW_NO_PREFIX_SHARE");
  c.nw_dedup_min_n = env_i64("DYNAALIGN_NW_DEDUP_MIN_N", -1);
  c.no_host_widen = env_flag("DYNAALIGN_NO_HOST_WIDEN");
  c.plain_d2h = env_flag("DYNAALIGN_PLAIN_D2H");
  c.no_buffer_cache = env_flag("DYNAALIGN_NO_BUFFER_CACHE");
  c.d2h_threads = (int)std::max<int64_t>(0, env_i64("DYNAALIGN_D2H_THREADS", 0));
  c.buffer_cache_pct = (int)std::max<int64_t>(0, std::min<int64_t>(90, env_i64("DYNAALIGN_BUFFER_CACHE_PCT", 30)));
  c.block_bytes = env_u64("DYNAALIGN_BLOCK_BYTES", 0);
  c.trace = env_flag("DYNAALIGN_TRACE");
  c.louvain_debug = env_flag("DYNAALIGN_LOUVAIN_DEBUG");
  c.louvain_threads = (int)std::max<int64_t>(0, env_i64("DYNAALIGN_LOUVAIN_THREADS", 0));
  c.cc_blocks = (int)std::max<int64_t>(0, std::min<int64_t>(1 << 16, env_i64("DYNAALIGN_CC_BLOCKS", 0)));
  return c;
}
std::atomic<const Config *> g_config{nullptr};
}  // namespace
const Config &config() {
  const Config *c = g_config.load(std::memory_order_acquire);
  if (!c) {
    const Config *fresh = new Config(parse_config());
    if (g_config.compare_exchange_strong(c, fresh, std::memory_order_acq_rel)) c = fresh;
    else delete fresh;
  }
  return *c;
}
}  // namespace da
// test hook: parse the environment again (the previous struct stays allocated: another host thread may still be reading it)
extern "C" void da_config_reload(void) { da::g_config.store(new da::Config(da::parse_config()), std::memory_order_release); }

extern "C" {

const char *da_last_error(void) { return last_error_ref().c_str(); }

const char *da_status_message(int status) {
  switch (status) {
    case DA_ERR_EMPTY_INPUT: return "Input sequences vector cannot be empty";      // src/minHash.cpp:122
    case DA_ERR_BAD_K: return "'k' must be a positive integer";                   // src/minHash.cpp:126
    case DA_ERR_BAD_NHASH: return "Number of hash functions must be positive";     // src/minHash.cpp:130
    case DA_ERR_BAD_MATRIX: return "Invalid substitution matrix name: %s";         // src/pairwiseSeqAlign.cpp:204
    case DA_ERR_BAD_RESIDUE_SEQ1: return "Invalid amino acid in sequence1: %c";    // :242
    case DA_ERR_BAD_RESIDUE_SEQ2: return "Invalid amino acid in sequence2: %c";    // :249
    case DA_ERR_NOMEM: return "out of memory";
    case DA_ERR_NO_DEVICE: return "no usable HIP device";
    case DA_ERR_HIP: return "HIP runtime error";
    case DA_ERR_UNSUPPORTED: return "unsupported by the gfx950 kernels";
    case DA_ERR_BAD_ARG: return "bad argument";
    default: return "";
  }
}

int da_abi_version(void) { return DA_ABI_VERSION; }

size_t da_release_device_memory(void) {
  (void)da::destroy_cached_comms();          // cached RCCL communicators (multi-device entry points) go too
  return big_cache().release(-1);
}

int da_device_count(void) {
  int cnt = 0;
  if (hipGetDeviceCount(&cnt) != hipSuccess) return 0;
  return cnt;
}

// std::mt19937 restated (ISO C++ [rand.predef]); the reference draws the seeds
// through uniform_int_distribution<uint32_t> over the full range, which returns
// the raw engine output on libstdc++ (reference src/minHash.cpp:75-80).
int da_hash_family_seeds(uint32_t seed, int n_hash, uint32_t *seeds_out) {
  if (n_hash < 0 || (n_hash > 0 && !seeds_out)) return fail(DA_ERR_BAD_ARG, "bad n_hash / seeds_out");
  uint32_t s[624];
  s[0] = seed;
  for (uint32_t i = 1; i < 624; ++i) s[i] = 1812433253u * (s[i - 1] ^ (s[i - 1] >> 30)) + i;
  int pos = 624;
  for (int o = 0; o < n_hash; ++o) {
    if (pos == 624) {
      for (int i = 0; i < 624; ++i) {
        const uint32_t y = (s[i] & 0x80000000u) | (s[(i + 1) % 624] & 0x7fffffffu);
        s[i] = s[(i + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
      }
      pos = 0;
    }
    uint32_t y = s[pos++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    seeds_out[o] = y;
  }
  return DA_OK;
}

uint32_t da_random_seed(void) { return std::random_device{}(); }  // src/minHash.cpp:73

int da_matrix_id(const char *matrix_name) {
  if (matrix_name)
    for (int i = 0; i < matrix_count_host(); ++i)
      if (strcmp(matrix_name, matrix_name_host(i)) == 0) return i;
  fail(DA_ERR_BAD_MATRIX, "Invalid substitution matrix name: %s", matrix_name ? matrix_name : "");
  return -1;
}

// --------------------------------------------------------------- dev entry

int da_dev_minhash_signatures(const uint8_t *d_residues, const int64_t *d_offsets, int64_t n,
                              int64_t total_residues, int64_t max_len, int k, int n_hash,
                              const uint32_t *d_seeds, uint32_t *d_sig, int64_t ld_sig, void *stream) {
  (void)total_residues; (void)max_len;
  int rc = validate_mh(n, k, n_hash);
  if (rc != DA_OK) return rc;
  if (!d_residues || !d_offsets || !d_seeds || !d_sig) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (ld_sig < n_hash) return fail(DA_ERR_BAD_ARG, "ld_sig (%lld) < n_hash (%d)", (long long)ld_sig, n_hash);
  return launch_minhash_signatures(d_residues, d_offsets, n, k, n_hash, d_seeds, d_sig, ld_sig,
                                   static_cast<hipStream_t>(stream));
}

// signatures -> compare operand: dictionary codes (16 planes / group) when n allows, raw values otherwise
static int env_plane_bits() { return da::config().plane_bits; }   // DYNAALIGN_PLANE_BITS: 32 = raw planes, 12 / 16 = at least that many code planes
// Step 1: the column dictionaries (launch_mh_dictionary), read back -- run when n allows and codes are wanted (min_bits != 32).  ok: every column's
// values got codes; max_ids: the largest column's repeated values; bits_data: the code planes they need.  Synchronises `stream`.
struct Dictionary { bool ok = false; int max_ids = 0, bits_data = 32; int *d_status = nullptr; };
static int run_dictionary(const uint32_t *d_sig, int64_t ld_sig, int64_t n, int n_hash, int min_bits, void *d_work, size_t work_bytes,
                          Dictionary *dict, hipStream_t stream) {
  if (n > DA_DICT_MAX_N || min_bits == 32) return DA_OK;
  if (!d_work || work_bytes < mh_planes_workspace_bytes(n, n_hash))
    return fail(DA_ERR_BAD_ARG, "workspace smaller than da_mh_planes_workspace_bytes(n, n_hash)");
  int rc;
  if ((rc = launch_mh_dictionary(d_sig, ld_sig, n, n_hash, d_work, &dict->d_status, stream)) != DA_OK) return rc;
  int status[2] = {0, 0};
  DA_HIP_TRY(hipMemcpyAsync(status, dict->d_status, sizeof(status), hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipStreamSynchronize(stream));
  dict->ok = status[0] == 0; dict->max_ids = status[1];
  dict->bits_data = dict->ok ? mh_plane_bits_for(status[1]) : 32;
  return DA_OK;
}
// Step 2: codes -> planes (at least min_bits of them) when the dictionary gave codes, raw signature bits otherwise
static int planes_from(const Dictionary &dict, const uint32_t *d_sig, int64_t ld_sig, int64_t n, int n_hash, int min_bits, const void *d_work,
                       uint32_t *d_planes, int *bits_out, hipStream_t stream) {
  *bits_out = dict.ok ? std::max(dict.bits_data, min_bits) : 32;
  return dict.ok ? launch_ids_to_planes(d_work, n, n_hash, *bits_out, d_planes, stream) : launch_sig_to_planes(d_sig, ld_sig, n, n_hash, d_planes, stream);
}
// min_bits: 0 = as few code planes as the data needs, 12 / 16 = at least that many, 32 = raw planes
static int build_planes(const uint32_t *d_sig, int64_t ld_sig, int64_t n, int n_hash, int min_bits, void *d_work,
                        size_t work_bytes, uint32_t *d_planes, int *bits_out, hipStream_t stream) {
  min_bits = std::max(min_bits, env_plane_bits());
  Dictionary dict;
  const int rc = run_dictionary(d_sig, ld_sig, n, n_hash, min_bits, d_work, work_bytes, &dict, stream);
  return rc != DA_OK ? rc : planes_from(dict, d_sig, ld_sig, n, n_hash, min_bits, d_work, d_planes, bits_out, stream);
}

size_t da_mh_planes_workspace_bytes(int64_t n, int n_hash) { return mh_planes_workspace_bytes(n, n_hash); }
int64_t da_mh_planes_words(int64_t n, int n_hash) { return mh_planes_words(n, n_hash); }

int da_dev_mh_planes(const uint32_t *d_sig, int64_t ld_sig, int64_t n, int n_hash, int min_plane_bits, void *d_work,
                     size_t work_bytes, uint32_t *d_planes, int64_t planes_words, int *plane_bits_out, void *stream) {
  if (n <= 0) return fail(DA_ERR_EMPTY_INPUT, "%s", da_status_message(DA_ERR_EMPTY_INPUT));
  if (n_hash <= 0) return fail(DA_ERR_BAD_NHASH, "%s", da_status_message(DA_ERR_BAD_NHASH));
  if (!d_sig || !d_planes || !plane_bits_out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  if (ld_sig < n_hash) return fail(DA_ERR_BAD_ARG, "ld_sig (%lld) < n_hash (%d)", (long long)ld_sig, n_hash);
  if (min_plane_bits != 0 && min_plane_bits != 12 && min_plane_bits != 14 && min_plane_bits != 15 && min_plane_bits != 16 && min_plane_bits != 32)
    return fail(DA_ERR_BAD_ARG, "min_plane_bits must be 0, 12, 14, 15, 16 or 32 (got %d)", min_plane_bits);
  if ((reinterpret_cast<uintptr_t>(d_planes) & 15) || planes_words < mh_planes_words(n, n_hash))
    return fail(DA_ERR_BAD_ARG, "bit-plane buffer must be 16-byte aligned and hold da_mh_planes_words(n, n_hash) = %lld words",
                (long long)mh_planes_words(n, n_hash));
  if (reinterpret_cast<uintptr_t>(d_work) & 255) return fail(DA_ERR_BAD_ARG, "workspace must be 256-byte aligned");
  return build_planes(d_sig, ld_sig, n, n_hash, min_plane_bits, d_work, work_bytes, d_planes, plane_bits_out,
                      static_cast<hipStream_t>(stream));
}

int da_dev_mh_compare(const uint32_t *d_planes, int plane_bits, int64_t n, int n_hash,
                      int64_t row_begin, int64_t row_end, int symmetric, int kind, void *d_out,
                      int64_t ld, void *stream) {
  if (n <= 0) return fail(DA_ERR_EMPTY_INPUT, "%s", da_status_message(DA_ERR_EMPTY_INPUT));
  if (n_hash <= 0) return fail(DA_ERR_BAD_NHASH, "%s", da_status_message(DA_ERR_BAD_NHASH));
  if (!d_planes || !d_out) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (row_begin < 0 || row_end > n || row_begin > row_end) return fail(DA_ERR_BAD_ARG, "bad row range");
  if (symmetric && (row_begin != 0 || row_end != n))
    return fail(DA_ERR_BAD_ARG, "symmetric mode needs the full row range");
  if (ld < n) return fail(DA_ERR_BAD_ARG, "ld (%lld) < n (%lld)", (long long)ld, (long long)n);
  if (kind != DA_OUT_F64 && kind != DA_OUT_COMPACT) return fail(DA_ERR_BAD_ARG, "bad output kind");
  if (n_hash > 65535)
    return fail(DA_ERR_UNSUPPORTED, "the compare kernel counts in 16 bits: n_hash <= 65535 (got %d)", n_hash);
  if (reinterpret_cast<uintptr_t>(d_planes) & 15) return fail(DA_ERR_BAD_ARG, "bit-plane buffer must be 16-byte aligned");
  if (plane_bits != 8 && plane_bits != 12 && plane_bits != 14 && plane_bits != 15 && plane_bits != 16 && plane_bits != 32)
    return fail(DA_ERR_BAD_ARG, "plane_bits must be 8, 12, 14, 15, 16 or 32 (got %d)", plane_bits);
  return launch_mh_compare(d_planes, n, n_hash, row_begin, row_end, symmetric != 0, kind, d_out, ld,
                           static_cast<hipStream_t>(stream), plane_bits);
}

// similarityMH, packed residues in HBM -> dense float64 n x n in HBM, as ONE call (K1 + K1b + K2 and the route below).
// Byte-identical sequences have identical signatures, hence identical rows and columns of the result: when at least 15 % of the
// sequences are duplicates the pipeline runs on the table of U unique strings (the plan of the NW route: nw_kernels.hip
// "duplicate sequences"; MinHash similarity IS symmetric, so the plain symmetric compare on U rows does) -- K2's work shrinks by
// (U/n)^2 -- and the n x n matrix is an index expansion of the U x U count table (launch_expand_unique's two streaming passes,
// 5.7 TB/s of stores).  Exact.  Taken when at most 60 % of the sequences are unique (below that K2's saving outweighs the expansion);
// otherwise (uniform peptides: nothing to collapse), or when the expansion's fast passes do not cover the shape
// (U > 65536, n_hash > 2047, n < 2048), the direct kernels run.  Synchronises `stream` (K1b reads the dictionary sizes back).
// DYNAALIGN_MH_NO_DEDUP=1 switches the route off.
namespace {
// side stream + events of the pipelined form, pooled per device (creating them costs more than the route's small kernels)
struct PipeRes { hipStream_t side = nullptr, alt[2] = {nullptr, nullptr}; std::vector<hipEvent_t> ev; int dev = 0; };
struct PipePool { std::mutex m; std::vector<PipeRes *> idle[64]; };
static PipePool &pipe_pool() { static PipePool *p = new PipePool; return *p; }   // never destroyed: the HIP runtime may be gone at exit
static PipeRes *pipe_acquire(size_t events) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  PipeRes *r = nullptr;
  {
    std::lock_guard<std::mutex> g(pipe_pool().m);
    auto &v = pipe_pool().idle[dev & 63];
    if (!v.empty()) { r = v.back(); v.pop_back(); }
  }
  if (!r) {
    r = new PipeRes;
    r->dev = dev;
    if (hipStreamCreateWithFlags(&r->side, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithFlags(&r->alt[0], hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&r->alt[1], hipStreamNonBlocking) != hipSuccess) { delete r; return nullptr; }
  }
  while (r->ev.size() < events) {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) break;
    r->ev.push_back(e);
  }
  if (r->ev.size() < events) { std::lock_guard<std::mutex> g(pipe_pool().m); pipe_pool().idle[dev & 63].push_back(r); return nullptr; }
  return r;
}
// a PipeRes held by one form (r: nullptr if none wanted / to be had); drains its streams, so declare it after the buffers they use
struct PipeLease {
  PipeRes *const r;
  explicit PipeLease(size_t events, bool want = true) : r(want ? pipe_acquire(events) : nullptr) {}
  ~PipeLease() {
    if (!r) return;
    (void)hipStreamSynchronize(r->side); (void)hipStreamSynchronize(r->alt[0]); (void)hipStreamSynchronize(r->alt[1]);
    std::lock_guard<std::mutex> g(pipe_pool().m);
    pipe_pool().idle[r->dev & 63].push_back(r);
  }
};
// the unique strings of a plan laid out by nw_dedup_layout: launch_nw_dedup_count, *U = M + S read back (synchronises `stream`)
static int count_unique(const uint8_t *d_bytes, const int64_t *d_offsets, int64_t n, const NwDedupPlan &p, hipStream_t stream, int64_t *U) {
  int rc;
  if ((rc = launch_nw_dedup_count(d_bytes, d_offsets, n, p, stream)) != DA_OK) return rc;
  int32_t M = 0, S = 0;
  DA_HIP_TRY(hipMemcpyAsync(&M, p.pm + n, 4, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipMemcpyAsync(&S, p.ps + n, 4, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipStreamSynchronize(stream));
  *U = (int64_t)M + S; return DA_OK;
}
enum MhForm { MH_DIRECT = 0, MH_TILES = 1, MH_SPARSE = 2, MH_TILES_PIPE = 3, MH_ROWS = 4, MH_ROWS_PIPE = 5 };   // da_mh_last_route's `taken`
struct MhRoute { int64_t n = 0, unique = 0, hybrid_pairs = -1; int taken = MH_DIRECT, plane_bits = 0, chunks = 0, expand_launches = 0, hybrid_bits_before = 0, dedup_order = -1; bool packed_table = false; float ms[6] = {0, 0, 0, 0, 0, 0}; };   // plan, K1 + K1b, K2, column gather, k_expand_rows, diagonal / border tiles
static MhRoute &mh_route() { static thread_local MhRoute r; return r; }
// the seven events of one call: [0] call, [1] plan done, [2] compare operand done, [3 ..] the form's own
struct MhEvents {
  hipEvent_t e[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  ~MhEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
  hipEvent_t operator[](int i) const { return e[i]; }
  static void ms(MhRoute &r, int i, hipEvent_t from, hipEvent_t to) { (void)hipEventElapsedTime(&r.ms[i], from, to); }
  void steps(MhRoute &r, int count) const { for (int i = 0; i < count; ++i) ms(r, i, e[i], e[i + 1]); }   // ms[i] = e[i] -> e[i + 1]
};
// ms[4] of the pipelined forms: the time some expansion launch was running -- the launches (in order) overlap on the alternating streams, so
// the union of their [begin, end) intervals, not the sum
struct LaunchUnion {
  hipEvent_t origin; float total = 0, covered_to = 0;
  void add(hipEvent_t begin, hipEvent_t end) {
    float b = 0, e = 0;
    (void)hipEventElapsedTime(&b, origin, begin); (void)hipEventElapsedTime(&e, origin, end);
    if (e > covered_to) { total += e - std::max(b, covered_to); covered_to = e; }
  }
};
// The duplicate plan: U unique strings; when collapsed (`take`), the expansion family (`rows`: k_expand_stream, else tiles) and the ids -- the
// row forms': zoned (DedupOrder; DYNAALIGN_MH_DEDUP_ORDER=first|zoned), so that every band of table rows the compare finishes unlocks about as
// many items in each zone of the expansion; the tiles': by first occurrence, with ub[b] = unique ids the input rows [0, 1024 b) use (the plan's
// prefix counts at band boundaries): the tile pipeline's schedule
struct MhDedup { int64_t U = 0; bool take = false, rows = false; DedupOrder order = DedupOrder::first; DevBuf work; NwDedupPlan p{}; std::vector<int32_t> ub; };
// the first half of every MinHash duplicate plan: the plan's workspace and the number of unique strings (synchronises `stream`)
static int mh_count_unique(const uint8_t *d_res, const int64_t *d_off, int64_t n, int64_t total, DevBuf *work, NwDedupPlan *p, int64_t *U,
                           hipStream_t stream) {
  int rc;
  if ((rc = work->alloc(nw_dedup_workspace_bytes(n, total))) != DA_OK) return rc;
  *p = nw_dedup_layout(work->p, n, total);
  return count_unique(d_res, d_off, n, *p, stream, U);
}
static int mh_dedup_plan(const uint8_t *d_res, const int64_t *d_off, int64_t n, int64_t total, int n_hash, const double *d_out, int64_t ld,
                         MhDedup *d, hipStream_t stream) {
  const Config &cfg = da::config();
  int rc;
  d->U = n;
  const int64_t min_n = cfg.mh_dedup_min_n >= 0 ? cfg.mh_dedup_min_n : 2048;   // DYNAALIGN_MH_DEDUP_MIN_N: tests lower it to reach the route with small inputs
  if (n < min_n || n > 0x7ffffff0LL || total <= 0 || n_hash > 2047 || cfg.mh_no_dedup) return DA_OK;
  if ((rc = mh_count_unique(d_res, d_off, n, total, &d->work, &d->p, &d->U, stream)) != DA_OK) return rc;
  const int64_t U = d->U;
  // K2 on U rows + column gather + expansion (0.5 + 1.6 f + 22 f^2 + 4.1 f + 14.4 ms at N = 100k, f = U / n) against K1 + K1b + K2 with its
  // own float64 stores (27.2 ms): the route pays below f = 0.63
  // ... with the tile expansion.  With the row expansion (no gather, no copy of the table) the route costs ~1.5 + 26 f^2 + 14 ms one kernel after the
  // other: 24.4 ms at f = 0.60, 26.6 at f = 0.65 against 27 (12 code planes) - 30 ms (14) for the direct kernels (profiles/r03_q_dedup_threshold.txt): 0.68
  const int64_t max_pct = cfg.mh_dedup_max_pct >= 0 ? cfg.mh_dedup_max_pct                             // DYNAALIGN_MH_DEDUP_MAX_PCT
                        : expand_stream_ok(n, std::min<int64_t>(U, 65536), n_hash, d_out, ld) ? 68 : 60;
  d->take = U > 0 && U * 100 <= n * max_pct && expand_rows_workspace_bytes(n, U, DA_OUT_F64, false, n_hash, 0) != 0;
  if (!d->take) return DA_OK;
  d->rows = cfg.mh_expand <= MH_EXPAND_ROWSPIPE && expand_stream_ok(n, U, n_hash, d_out, ld);
  // The row forms take table rows in id order and output rows by zone: the zoned ids put the strings with copies all over the matrix first and
  // spread every zone's single-copy strings evenly over the remaining table rows.  The matrix does not depend on the numbering.
  d->order = d->rows && cfg.mh_dedup_order != 1 ? DedupOrder::zoned : DedupOrder::first;
  if ((rc = launch_nw_dedup_build(d_res, d_off, n, U, d->p, stream, d->order, d->rows ? expand_stream_zones() : 1)) != DA_OK) return rc;
  if (d->rows) return DA_OK;
  const int64_t NB = mh_sym_bands(n);
  std::vector<int32_t> b((size_t)NB);
  d->ub.resize((size_t)NB + 1);
  DA_HIP_TRY(hipMemcpy2DAsync(d->ub.data(), 4, d->p.pm, 4096, 4, (size_t)NB, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipMemcpy2DAsync(b.data(), 4, d->p.ps, 4096, 4, (size_t)NB, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipStreamSynchronize(stream));
  for (int64_t q = 0; q < NB; ++q) d->ub[(size_t)q] += b[(size_t)q];
  d->ub[(size_t)NB] = (int32_t)U;
  return DA_OK;
}
// Admission of the two ways around comparing every code plane.  Sparse (minhash_kernels.hip "SPARSE route"): the signatures rarely agree --
// no planes, the matching incidences are enumerated from the dictionary codes.  Split (dict_kernels.hip k_hy_split): 12 - 16 code planes, but all
// except a few matching incidences sit on each column's HY_KEEP most frequent values -- EIGHT planes of dense codes for those, and the rare
// values' codes go to launch_mh_sparse_lists and, after the dense compare, launch_mh_sparse_fixup.
constexpr int HY_KEEP = 254;
enum class MhOperand { dense, sparse, split };
// pairs: matching (sparse) / rare (split) incidences; codes: what the list kernels read (all / the rare codes); dense: the split's dense codes
struct MhAdmission { MhOperand form = MhOperand::dense; uint64_t pairs = 0; const uint16_t *codes = nullptr, *dense = nullptr; int64_t ld_ids = 0; };
static int mh_admit(const Dictionary &dict, void *d_work, int64_t n, int n_hash, bool ask_sparse, int split_from_bits, MhAdmission *a,
                    hipStream_t stream) {
  const Config &cfg = da::config();
  if (!dict.ok || env_plane_bits() != 0) return DA_OK;              // both need codes, and no more planes than the data needs
  // below n = 16384 the compare is too short to pay for the list kernels (DYNAALIGN_MH_HYBRID_MIN_N: tests lower it)
  const int64_t hy_min_n = cfg.mh_hybrid_min_n >= 0 ? cfg.mh_hybrid_min_n : 16384;
  const bool sparse_ok = ask_sparse && dict.max_ids >= 1 && dict.max_ids <= 32768 && n >= 2048 && n_hash + 1 <= 2048 && !cfg.mh_no_sparse;
  const bool split_ok = dict.bits_data >= split_from_bits && dict.bits_data <= 16 && dict.max_ids <= 32768 && n >= hy_min_n && n <= 131072 &&
                        n_hash > 32 && n_hash + 1 <= 2048 && !cfg.mh_no_hybrid && !cfg.k2_no_asm;
  if (!sparse_ok && !split_ok) return DA_OK;
  // how many (pair, hash function) incidences match, and how large is the largest class -- over all repeated values (sparse route) and over the values
  // outside each column's HY_KEEP most frequent ones (heavy / rare split)?
  int rc;
  int64_t ld_ids = 0;
  const uint16_t *ids = mh_dictionary_codes(d_work, n, n_hash, &ld_ids);
  unsigned long long *d_stats = reinterpret_cast<unsigned long long *>(dict.d_status + 4);     // behind the two status words (the workspace ends 256 bytes later)
  const uint16_t *dense = nullptr, *rare = nullptr;
  unsigned long long st[4] = {0, 0, 0, 0};                          // rare incidences, largest rare class, all incidences, largest class
  if ((rc = split_ok ? launch_mh_heavy_split(d_work, n, n_hash, dict.max_ids, HY_KEEP, &dense, &rare, d_stats, stream)
                     : launch_mh_sparse_count(ids, ld_ids, n, n_hash, dict.max_ids, d_stats, stream)) != DA_OK) return rc;
  DA_HIP_TRY(hipMemcpyAsync(split_ok ? st : st + 2, d_stats, split_ok ? sizeof(st) : 16, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipStreamSynchronize(stream));
  const double pairs_all = 0.5 * (double)n * (double)(n - 1);
  // sparse: the bucket phase costs ~37 ps per incidence (5.1 ms for 1.37e8) and the tile pass ~2.5 ps per pair, the dense compare ~6.3 ps
  // per pair at n_hash = 500 -- so the route pays while the average number of matches per pair stays below ~0.1 (x n_hash / 500);
  // plus a memory cap on the bucket and a cap on the class size (a thread walks its class)
  if (sparse_ok && st[2] <= mh_sparse_pairs_limit() && st[3] <= 4096 && (double)st[2] <= pairs_all * (double)n_hash / 5000.0)
    *a = MhAdmission{MhOperand::sparse, st[2], ids, nullptr, ld_ids};
  // split: four to eight planes less = 30 - 47 % of the compare's plane work (~2 ps per pair and 4 planes at n_hash = 500), against
  // ~37 ps per rare incidence in the list kernels + ~1 ms of fixed cost: taken while the rare values match in < 0.02 of the pairs (x n_hash / 500)
  else if (split_ok && st[0] <= mh_sparse_pairs_limit() && st[1] <= 4096 && (double)st[0] <= pairs_all * (double)n_hash / 25000.0)
    *a = MhAdmission{MhOperand::split, st[0], rare, dense, ld_ids};
  return DA_OK;
}
// The compare operand for `m` rows (K1 + K1b and the admission above) and the list kernels' scratch of the sparse route and the split
struct MhCodes {
  DevBuf sig, planes, pwork, scratch, entries32, entries;
  int64_t m = 0;
  int n_hash = 0, bits = 32;   // the planes built (0: none, the sparse route)
  Dictionary dict;
  MhAdmission adm;
  bool split() const { return adm.form == MhOperand::split; }
  // lists of the rare values' incidences (tile by tile) and, after a compare, their addition to its result (tile rows [tr0, tr1), all by default)
  int lists(hipStream_t st) const {
    return launch_mh_sparse_lists(adm.codes, adm.ld_ids, m, n_hash, dict.max_ids, adm.pairs, scratch.as<uint32_t>(), entries32.as<uint32_t>(), entries.as<uint16_t>(), st);
  }
  int fixup(int kind, void *out, int64_t ld_out, hipStream_t st, int64_t tr0 = 0, int64_t tr1 = -1) const {
    return launch_mh_sparse_fixup(scratch.as<uint32_t>(), entries.as<uint16_t>(), m, n_hash, dict.max_ids, adm.ld_ids, kind, out, ld_out, tr0,
                                  tr1 < 0 ? (m + 127) / 128 : tr1, st);
  }
};
static int mh_codes(const uint8_t *d_res, const int64_t *d_off, int64_t m, int k, int n_hash, const uint32_t *d_seeds, bool ask_sparse,
                    int split_from_bits, MhCodes *c, hipStream_t stream) {
  int rc;
  const int64_t lds = sig_ld_for(n_hash);
  const size_t wb = mh_planes_workspace_bytes(m, n_hash);
  c->m = m; c->n_hash = n_hash;
  if ((rc = c->sig.alloc((size_t)m * lds * sizeof(uint32_t))) != DA_OK || (rc = c->planes.alloc((size_t)mh_planes_words(m, n_hash) * sizeof(uint32_t))) != DA_OK ||
      (rc = c->pwork.alloc(wb)) != DA_OK) return rc;
  uint32_t *sig = c->sig.as<uint32_t>(), *planes = c->planes.as<uint32_t>();
  if ((rc = launch_minhash_signatures(d_res, d_off, m, k, n_hash, d_seeds, sig, lds, stream)) != DA_OK) return rc;
  const int min_bits = env_plane_bits();
  const Dictionary &dict = c->dict;
  if ((rc = run_dictionary(sig, lds, m, n_hash, min_bits, c->pwork.p, wb, &c->dict, stream)) != DA_OK) return rc;
  if ((rc = mh_admit(dict, c->pwork.p, m, n_hash, ask_sparse, split_from_bits, &c->adm, stream)) != DA_OK) return rc;
  // Both forms are optimisations: when the lists' scratch does not fit, what did allocate goes back and the dense planes are built instead.
  // Those are the planes of a full build_planes -- the dictionary's codes at bits_data: both forms are admitted only when DYNAALIGN_PLANE_BITS
  // leaves min_bits == 0, and k_hy_split writes its codes to the sort scratch (w.sz / w.si), so the dictionary's codes (idsT) in pwork are intact.
  if (c->adm.form != MhOperand::dense &&
      (c->scratch.alloc(mh_sparse_scratch_words(m, n_hash, dict.max_ids, c->adm.ld_ids) * 4) != DA_OK ||
       c->entries32.alloc((size_t)c->adm.pairs * 4 + 16) != DA_OK || c->entries.alloc((size_t)c->adm.pairs * 2 + 16) != DA_OK)) {
    (void)hipGetLastError();
    c->scratch.release(); c->entries32.release(); c->entries.release();
    c->adm = MhAdmission();
  }
  if (c->adm.form == MhOperand::sparse) { c->bits = 0; return DA_OK; }
  if (c->split()) { c->bits = 8; return launch_ids_to_planes(c->pwork.p, m, n_hash, 8, planes, stream, c->adm.dense); }
  return planes_from(dict, sig, lds, m, n_hash, min_bits, c->pwork.p, planes, &c->bits, stream);
}
// what the forms share; duplicate route: the U x U count table (ld_d) and the expansion's scratch (copy lists / column-gathered table).
// pk: the table is packed to 9 bits per count (da_common.hpp pk_*, ld_d = its low plane's bytes): the row forms with n_hash <= 511, 12 planes
// and no heavy / rare split (k_hy_fixup adds into uint16 entries)
struct MhCall {
  int64_t n; int n_hash; double *out; int64_t ld; hipStream_t stream; MhRoute &route; const MhEvents &ev; const MhCodes &c; const MhDedup &d;
  uint16_t *dtab = nullptr; int64_t ld_d = 0; void *ex = nullptr; bool pk = false;
};
constexpr int MH_NO_PIPE = -1;   // a pipelined form's return when no side stream / events are to be had: the one-stream form needs none
// the end of every form: its last event on the caller's stream, the sync after which the buffers may go back to the cache, the route report
static int mh_finish(const MhCall &k, int last_event, MhForm taken, int steps) {
  DA_HIP_TRY(hipEventRecord(k.ev[last_event], k.stream));
  DA_HIP_TRY(hipStreamSynchronize(k.stream));
  k.route.taken = taken; k.ev.steps(k.route, steps);
  return DA_OK;
}
// SPARSE route: the matching incidences are enumerated from the dictionary codes, bucketed per output tile and every tile written once (exact;
// minhash_kernels.hip).  ms[2] = link + walk + scan (buckets), ms[4] = the tile pass.
static int mh_sparse(const MhCall &k) {
  const MhCodes &c = k.c;
  int rc;
  if ((rc = launch_mh_sparse(c.adm.codes, c.adm.ld_ids, k.n, k.n_hash, c.dict.max_ids, c.adm.pairs, c.scratch.as<uint32_t>(), c.entries32.as<uint32_t>(),
                             c.entries.as<uint16_t>(), k.out, k.ld, k.stream, k.ev[3])) != DA_OK || (rc = mh_finish(k, 4, MH_SPARSE, 3)) != DA_OK) return rc;
  k.route.unique = (int64_t)c.adm.pairs;                            // (reported as `sparse_pairs` by the Python wrapper)
  MhEvents::ms(k.route, 4, k.ev[3], k.ev[4]);
  return DA_OK;
}
// the direct kernels on all n rows; the split's list kernels (latency-bound, ~0.9 ms at 100k) run on a side stream beside the dense compare,
// without a side stream before it
static int mh_direct(const MhCall &k) {
  const MhCodes &c = k.c;
  int rc;
  const PipeLease lease(1, c.split());
  PipeRes *const pr = lease.r;
  if (pr) {
    DA_HIP_TRY(hipStreamWaitEvent(pr->side, k.ev[2], 0));
    if ((rc = c.lists(pr->side)) != DA_OK) return rc;
    DA_HIP_TRY(hipEventRecord(pr->ev[0], pr->side));
  } else if (c.split() && (rc = c.lists(k.stream)) != DA_OK) return rc;
  if ((rc = launch_mh_compare(c.planes.as<uint32_t>(), k.n, k.n_hash, 0, k.n, true, DA_OUT_F64, k.out, k.ld, k.stream, c.bits)) != DA_OK) return rc;
  if (pr) DA_HIP_TRY(hipStreamWaitEvent(k.stream, pr->ev[0], 0));
  if (c.split() && (rc = c.fixup(DA_OUT_F64, k.out, k.ld, k.stream)) != DA_OK) return rc;
  return mh_finish(k, 3, MH_DIRECT, 3);
}
// The one-stream duplicate forms: K2 on the U unique rows into the count table (+ the split's lists and fix-up), then the expansion --
//   rows    k_expand_stream: every output row written once from its table row in LDS (no gathered copy); ms[3] = the copy lists (positions
//           of every id, work items), ms[4] = k_expand_stream
//   tiles   column gather (k_gather_columns), tile expansion (k_expand_rows) + diagonal / border tiles, one after the other
static int mh_one_stream(const MhCall &k) {
  const MhCodes &c = k.c;
  int rc;
  if (c.split() && (rc = c.lists(k.stream)) != DA_OK) return rc;
  if ((rc = k.pk ? launch_mh_compare_pk(c.planes.as<uint32_t>(), k.d.U, k.n_hash, reinterpret_cast<uint8_t *>(k.dtab), k.stream)
                 : launch_mh_compare(c.planes.as<uint32_t>(), k.d.U, k.n_hash, 0, k.d.U, true, DA_OUT_COMPACT, k.dtab, k.ld_d, k.stream, c.bits)) != DA_OK)
    return rc;
  if (c.split() && (rc = c.fixup(DA_OUT_COMPACT, k.dtab, k.ld_d, k.stream)) != DA_OK) return rc;
  DA_HIP_TRY(hipEventRecord(k.ev[3], k.stream));
  if ((rc = k.d.rows ? launch_expand_stream(k.dtab, k.ld_d, k.d.p.uidx, k.n, k.d.U, k.n_hash, k.out, k.ld, k.ex, k.stream, k.ev[4], k.pk)
                     : launch_expand_unique(k.dtab, k.ld_d, k.d.p.uidx, k.n, DA_OUT_F64, false, k.n_hash, k.out, k.ld, k.stream, 0,
                                            static_cast<uint16_t *>(k.ex), k.d.p.ufirst, k.d.U, k.ev[4], k.ev[5])) != DA_OK) return rc;
  k.route.chunks = k.route.expand_launches = 1;
  return k.d.rows ? mh_finish(k, 5, MH_ROWS, 5) : mh_finish(k, 6, MH_TILES, 6);
}
// rowspipe: the row expansion PIPELINED with K2 -- the first `head` bands of the table at full occupancy, the rest by the persistent kernel with
// `wg` workgroup(s) per CU on a side stream (one 36 KB ring fits beside the expansion's 94 KB row) while the finished table rows are expanded
static int mh_rows_pipe(const MhCall &k) {
  const Config &cfg = da::config();
  const MhCodes &c = k.c;
  const int64_t U = k.d.U, KB = mh_sym_bands(U);
  const hipStream_t stream = k.stream;
  int rc;
  // K2 rings (36 KB, 128 VGPRs x 4 waves) that fit beside one expansion workgroup: two when its LDS row is packed (n_hash <= 511), else one --
  // and a slower K2 wants a head start and smaller chunks (profiles/r03_m_pipeline_rows_*.txt: head x step sweeps for both)
  const bool two = expand_stream_packed(k.n_hash);
  const int wg = cfg.mh_pipe_wg > 0 ? cfg.mh_pipe_wg : two ? 2 : 1, head = cfg.mh_pipe_head > 0 ? cfg.mh_pipe_head : two ? 1 : 4,
            step = cfg.mh_pipe_step > 0 ? cfg.mh_pipe_step : two ? 8 : 4;
  const bool alt = !cfg.mh_pipe_one_stream;   // DYNAALIGN_MH_PIPE_STEP / _WG / _HEAD / _ONE_STREAM: schedule experiments
  std::vector<int64_t> cuts{0};
  while (cuts.back() < KB) cuts.push_back(std::min(KB, cuts.back() + (cuts.size() == 1 ? head : step)));
  const size_t C = cuts.size() - 1;
  const PipeLease lease(3 * C + 2);
  PipeRes *const pr = lease.r;
  if (!pr) return MH_NO_PIPE;
  hipEvent_t *pe = pr->ev.data();                                  // per chunk: table rows done, rows begin / end; [3 C]: lists done
  // beside the first band on the side stream: the table's diagonal / border tiles and the copy lists, both on the caller's stream
  DA_HIP_TRY(hipStreamWaitEvent(pr->side, k.ev[2], 0));
  if ((rc = launch_mh_compare_edges_u16(c.planes.as<uint32_t>(), U, k.n_hash, k.dtab, k.ld_d, stream, c.bits, k.pk)) != DA_OK) return rc;
  if ((rc = launch_expand_stream_lists(k.d.p.uidx, k.n, U, k.ex, stream)) != DA_OK) return rc;
  DA_HIP_TRY(hipEventRecord(pe[3 * C], stream));
  if (c.split()) {     // the rare values' lists behind them on the caller's stream (on the idle expansion stream instead: 17.3 vs 16.6 ms, round 4)
    if ((rc = c.lists(stream)) != DA_OK) return rc;
    DA_HIP_TRY(hipEventRecord(pe[3 * C + 1], stream));
  }
  if (alt) { DA_HIP_TRY(hipStreamWaitEvent(pr->alt[0], pe[3 * C], 0)); DA_HIP_TRY(hipStreamWaitEvent(pr->alt[1], pe[3 * C], 0)); }
  for (size_t ci = 0; ci < C; ++ci) {
    if ((rc = launch_mh_compare_bands_u16(c.planes.as<uint32_t>(), U, k.n_hash, k.dtab, k.ld_d, cuts[ci], cuts[ci + 1], ci == 0 ? 4 : wg, pr->side, c.bits,
                                          k.pk)) != DA_OK) return rc;
    if (c.split()) {     // the rare values' incidences of these tile rows (direct + mirrored elements), once the edge tiles and the lists are there
      if (ci == 0) { DA_HIP_TRY(hipStreamWaitEvent(pr->side, pe[3 * C], 0)); DA_HIP_TRY(hipStreamWaitEvent(pr->side, pe[3 * C + 1], 0)); }
      if ((rc = c.fixup(DA_OUT_COMPACT, k.dtab, k.ld_d, pr->side, cuts[ci] * 8, cuts[ci + 1] * 8)) != DA_OK) return rc;
    }
    DA_HIP_TRY(hipEventRecord(pe[3 * ci], pr->side));
    const hipStream_t es = alt ? pr->alt[ci & 1] : stream;
    DA_HIP_TRY(hipStreamWaitEvent(es, pe[3 * ci], 0));
    DA_HIP_TRY(hipEventRecord(pe[3 * ci + 1], es));
    // (the launches share the lists' ticket counters: this one takes the items of the finished table rows that the earlier ones left, the last
    // one whatever remains, its workgroups filling the CUs as older ones leave)
    if ((rc = launch_expand_stream_rows(k.dtab, k.ld_d, k.d.p.uidx, k.n, U, k.n_hash, k.out, k.ld, k.ex, cuts[ci + 1] * 1024, es, k.pk)) != DA_OK) return rc;
    DA_HIP_TRY(hipEventRecord(pe[3 * ci + 2], es));
  }
  if (alt) for (size_t ci = (C >= 2 ? C - 2 : 0); ci < C; ++ci) DA_HIP_TRY(hipStreamWaitEvent(stream, pe[3 * ci + 2], 0));
  if ((rc = mh_finish(k, 5, MH_ROWS_PIPE, 2)) != DA_OK) return rc;
  k.route.chunks = k.route.expand_launches = (int)C;
  MhEvents::ms(k.route, 2, k.ev[2], pe[3 * (C - 1)]);             // the compare's span on the side stream
  MhEvents::ms(k.route, 3, k.ev[2], pe[3 * C]);                   // the copy lists (beside the compare)
  LaunchUnion expand{k.ev[2]};
  for (size_t ci = 0; ci < C; ++ci) expand.add(pe[3 * ci + 1], pe[3 * ci + 2]);
  k.route.ms[4] = expand.total;
  return DA_OK;
}
// pipe: the PIPELINED tile form.  The table is compared band by band (1024 unique rows each, in order) by the persistent kernel
// on a side stream with only `wg` workgroups per CU, so the rest of every CU stays free; the output row bands whose strings are all numbered below
// the finished table rows are gathered (on `stream`) and expanded (on two alternating streams: chunk c + 1 fills the CUs as chunk c drains)
// meanwhile.  The compare is VALU work, the expansion store work; unique ids are numbered by first occurrence, so both sweep their triangles in
// the same direction and the compare stays ahead.  Same kernels, same bits.  Only diagonal / border tiles are left to launch_expand_unique.
static int mh_tiles_pipe(const MhCall &k) {
  const Config &cfg = da::config();
  const MhCodes &c = k.c;
  uint16_t *ftab = static_cast<uint16_t *>(k.ex);
  const hipStream_t stream = k.stream;
  const std::vector<int32_t> &ub = k.d.ub;
  const int64_t U = k.d.U, KB = mh_sym_bands(U), NB = (int64_t)ub.size() - 1, ld_f = ceil_div(k.n, 8) * 8;
  int rc;
  const int step = cfg.mh_pipe_step > 0 ? cfg.mh_pipe_step : 4, wg = cfg.mh_pipe_wg > 0 ? cfg.mh_pipe_wg : 2;
  const bool alt = !cfg.mh_pipe_one_stream;
  struct Chunk { int64_t kb0, kb1, ob0, ob1; };
  std::vector<Chunk> chunks;
  for (int64_t kb = 0, ob = 0; kb < KB;) {
    const int64_t kb1 = std::min(KB, kb + (chunks.empty() ? 1 : step));   // a first chunk of one band: the expansion starts early
    int64_t ob1 = ob;
    if (kb1 == KB) ob1 = NB;
    else while (ob1 < NB && (int64_t)ub[(size_t)ob1 + 1] <= kb1 * 1024) ++ob1;   // rows below 1024 (ob1 + 1) only use ids < ub[ob1 + 1]
    chunks.push_back({kb, kb1, ob, ob1});
    kb = kb1; ob = ob1;
  }
  const size_t C = chunks.size();
  const PipeLease lease(5 * C);
  PipeRes *const pr = lease.r;
  if (!pr) return MH_NO_PIPE;
  hipEvent_t *pe = pr->ev.data();                                  // per chunk: table rows done, gather begin / end, rows begin / end
  DA_HIP_TRY(hipStreamWaitEvent(pr->side, k.ev[2], 0));
  if ((rc = launch_mh_compare_edges_u16(c.planes.as<uint32_t>(), U, k.n_hash, k.dtab, k.ld_d, pr->side, c.bits)) != DA_OK) return rc;
  if (c.split() && (rc = c.lists(pr->side)) != DA_OK) return rc;
  for (size_t ci = 0; ci < C; ++ci) {
    const Chunk &ch = chunks[ci];
    if ((rc = launch_mh_compare_bands_u16(c.planes.as<uint32_t>(), U, k.n_hash, k.dtab, k.ld_d, ch.kb0, ch.kb1, wg, pr->side, c.bits)) != DA_OK) return rc;
    if (c.split() && (rc = c.fixup(DA_OUT_COMPACT, k.dtab, k.ld_d, pr->side, ch.kb0 * 8, ch.kb1 * 8)) != DA_OK) return rc;
    DA_HIP_TRY(hipEventRecord(pe[5 * ci], pr->side));
    DA_HIP_TRY(hipStreamWaitEvent(stream, pe[5 * ci], 0));
    DA_HIP_TRY(hipEventRecord(pe[5 * ci + 1], stream));
    if ((rc = launch_gather_columns(k.dtab, k.ld_d, k.d.p.uidx, k.d.p.ufirst, k.n, U, ftab, ld_f, false, stream, 1, 0, ch.kb0 * 1024,
                                    std::min(U, ch.kb1 * 1024))) != DA_OK) return rc;
    DA_HIP_TRY(hipEventRecord(pe[5 * ci + 2], stream));
    const hipStream_t es = alt ? pr->alt[ci & 1] : stream;
    if (alt) DA_HIP_TRY(hipStreamWaitEvent(es, pe[5 * ci + 2], 0));
    DA_HIP_TRY(hipEventRecord(pe[5 * ci + 3], es));
    if ((rc = launch_expand_rows(ftab, ld_f, k.d.p.uidx, k.n, false, k.n_hash, 0, k.out, k.ld, ch.ob0, ch.ob1, es)) != DA_OK) return rc;
    DA_HIP_TRY(hipEventRecord(pe[5 * ci + 4], es));
  }
  if (alt) for (size_t ci = (C >= 2 ? C - 2 : 0); ci < C; ++ci) DA_HIP_TRY(hipStreamWaitEvent(stream, pe[5 * ci + 4], 0));
  DA_HIP_TRY(hipEventRecord(k.ev[5], stream));
  if ((rc = launch_expand_unique(k.dtab, k.ld_d, k.d.p.uidx, k.n, DA_OUT_F64, false, k.n_hash, k.out, k.ld, stream, 0, ftab, k.d.p.ufirst, U,
                                 nullptr, nullptr, 1, 0, true)) != DA_OK) return rc;
  if ((rc = mh_finish(k, 6, MH_TILES_PIPE, 2)) != DA_OK) return rc;
  k.route.chunks = (int)C;
  MhEvents::ms(k.route, 2, k.ev[2], pe[5 * (C - 1)]);             // the compare's span on the side stream (it overlaps what follows)
  LaunchUnion expand{k.ev[2]};
  for (size_t ci = 0; ci < C; ++ci) {
    float g = 0;
    (void)hipEventElapsedTime(&g, pe[5 * ci + 1], pe[5 * ci + 2]);
    k.route.ms[3] += g;                                              // gathers: summed (each includes its wait for free LDS beside the expansion)
    if (chunks[ci].ob1 > chunks[ci].ob0) { ++k.route.expand_launches; expand.add(pe[5 * ci + 3], pe[5 * ci + 4]); }
  }
  k.route.ms[4] = expand.total;
  MhEvents::ms(k.route, 5, k.ev[5], k.ev[6]);
  return DA_OK;
}
}  // namespace

static int mh_full_symmetric(const uint8_t *d_res, const int64_t *d_off, int64_t n, int64_t total, int k, int n_hash,
                             const uint32_t *d_seeds, double *d_out, int64_t ld, hipStream_t stream) {
  const Config &cfg = da::config();
  int rc;
  MhRoute &route = mh_route() = MhRoute();
  route.n = n;
  MhEvents ev;
  for (auto &e : ev.e) DA_HIP_TRY(hipEventCreate(&e));
  DA_HIP_TRY(hipEventRecord(ev[0], stream));
  MhDedup d;
  if ((rc = mh_dedup_plan(d_res, d_off, n, total, n_hash, d_out, ld, &d, stream)) != DA_OK) return rc;
  route.unique = d.U;
  if (d.take) route.dedup_order = (int)d.order;
  DA_HIP_TRY(hipEventRecord(ev[1], stream));
  // sparse route: only with few duplicates (clustered inputs have large classes: the dense kernels win).  Split: the direct route; the duplicate
  // route's table when it needs more than 12 planes (no banded kernel for those: the split lets the route pipeline at all); with 12 planes the
  // pipelined route gains 0.2 ms of 16.8 from it at 100k (profiles/r04_l_*): on request only (DYNAALIGN_MH_HYBRID_DEDUP)
  MhCodes c;
  if ((rc = mh_codes(d.take ? d.p.ucodes : d_res, d.take ? d.p.uoff : d_off, d.take ? d.U : n, k, n_hash, d_seeds, !d.take && d.U * 10 >= n * 9,
                     d.take && !cfg.mh_hybrid_dedup ? 13 : 12, &c, stream)) != DA_OK) return rc;
  route.plane_bits = c.bits;
  if (c.split()) { route.hybrid_pairs = (int64_t)c.adm.pairs; route.hybrid_bits_before = c.dict.bits_data; }
  DA_HIP_TRY(hipEventRecord(ev[2], stream));
  MhCall call{n, n_hash, d_out, ld, stream, route, ev, c, d};
  if (!d.take) return c.adm.form == MhOperand::sparse ? mh_sparse(call) : mh_direct(call);
  // The expansion has two kernel families and each a pipelined form (DYNAALIGN_MH_EXPAND = rowspipe | rows | pipe | tiles; default: the first
  // whose shape test passes; DYNAALIGN_MH_NO_PIPE=1 takes the pipelined forms out)
  DevBuf dtab, ex;
  call.pk = d.rows && !c.split() && mh_compare_pk_ok(d.U, n_hash, c.bits);
  route.packed_table = call.pk;
  call.ld_d = call.pk ? pk_lo_bytes(d.U) : (d.U + 7) / 8 * 8;
  if ((rc = dtab.alloc(call.pk ? pk_table_bytes(d.U) : (size_t)d.U * (size_t)call.ld_d * 2)) != DA_OK) return rc;
  if ((rc = ex.alloc(d.rows ? expand_stream_scratch_bytes(n, d.U) : expand_rows_workspace_bytes(n, d.U, DA_OUT_F64, false, n_hash, 0))) != DA_OK) return rc;
  call.dtab = dtab.as<uint16_t>(); call.ex = ex.p;
  // (the pipelined tile form leaves only diagonal / border tiles to launch_expand_unique: the output must qualify for the streaming passes)
  const bool pipe = !cfg.mh_no_pipe && mh_compare_bands_ok(d.U, n_hash, c.bits, dtab.p, call.ld_d) &&
                    (d.rows ? cfg.mh_expand != MH_EXPAND_ROWS : cfg.mh_expand != MH_EXPAND_TILES && (ld & 1) == 0 && (reinterpret_cast<uintptr_t>(d_out) & 15) == 0);
  if (pipe && (rc = d.rows ? mh_rows_pipe(call) : mh_tiles_pipe(call)) != MH_NO_PIPE) return rc;
  return mh_one_stream(call);
}

int da_dev_similarity_mh(const uint8_t *d_residues, const int64_t *d_offsets, int64_t n, int64_t total_residues, int k, int n_hash,
                         const uint32_t *d_seeds, double *d_out, int64_t ld, void *stream) {
  int rc = validate_mh(n, k, n_hash);
  if (rc != DA_OK) return rc;
  if (!d_residues || !d_offsets || !d_seeds || !d_out) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (ld < n) return fail(DA_ERR_BAD_ARG, "ld (%lld) < n (%lld)", (long long)ld, (long long)n);
  if (n_hash > 65535) return fail(DA_ERR_UNSUPPORTED, "the compare kernel counts in 16 bits: n_hash <= 65535 (got %d); da_similarity_mh handles more", n_hash);
  return mh_full_symmetric(d_residues, d_offsets, n, total_residues, k, n_hash, d_seeds, d_out, ld, static_cast<hipStream_t>(stream));
}

int da_mh_last_route_chunks(int *chunks_out, int *expand_launches_out) {
  const MhRoute &r = mh_route();
  if (chunks_out) *chunks_out = r.chunks;
  if (expand_launches_out) *expand_launches_out = r.expand_launches;
  return DA_OK;
}

int da_mh_last_route_split(int64_t *rare_incidences_out, int *plane_bits_without_out) {
  const MhRoute &r = mh_route();
  if (rare_incidences_out) *rare_incidences_out = r.hybrid_pairs;
  if (plane_bits_without_out) *plane_bits_without_out = r.hybrid_bits_before;
  return DA_OK;
}

// tests: the id order (DedupOrder) of the calling thread's last similarityMH call, -1 when it did not collapse duplicates
extern "C" int da_debug_mh_last_dedup_order(int *order_out) {
  if (!order_out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  *order_out = mh_route().dedup_order;
  return DA_OK;
}
// tests: the duplicate plan's numbering.  Runs the count and the build for `order` (DedupOrder: 0 multi-copy first, 1 first occurrence, 2 zoned)
// with `zones` zones (0: what a call uses) on n sequences and copies the id of every sequence to d_uidx_out[n]; unique_out = U, multi_out = M, the
// multi-copy strings.  Synchronises `stream`.
extern "C" int da_debug_mh_dedup_ids(const uint8_t *d_res, const int64_t *d_off, int64_t n, int64_t total, int order, int zones, int32_t *d_uidx_out,
                                     int64_t *unique_out, int64_t *multi_out, void *stream) {
  if (zones == 0) zones = expand_stream_zones();
  if (!d_res || !d_off || !d_uidx_out || n < 1 || n > 0x7ffffff0LL || total <= 0 || order < 0 || order > 2 || zones < 1 || zones > ES_ZONES)
    return fail(DA_ERR_BAD_ARG, "dedup ids: bad arguments");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  DevBuf work;
  NwDedupPlan p{};
  int64_t U = 0;
  int32_t M = 0;
  int rc;
  if ((rc = mh_count_unique(d_res, d_off, n, total, &work, &p, &U, st)) != DA_OK) return rc;
  if ((rc = launch_nw_dedup_build(d_res, d_off, n, U, p, st, static_cast<DedupOrder>(order), zones)) != DA_OK) return rc;
  DA_HIP_TRY(hipMemcpyAsync(d_uidx_out, p.uidx, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
  DA_HIP_TRY(hipMemcpyAsync(&M, p.pm + n, 4, hipMemcpyDeviceToHost, st));
  DA_HIP_TRY(hipStreamSynchronize(st));
  if (unique_out) *unique_out = U;
  if (multi_out) *multi_out = M;
  return DA_OK;
}
// tests: the zoned order's id function on the host (da_common.hpp zoned_rank).  For zone sizes h[zones] and M multi-copy strings, the ids of
// all (z, q), q < h[z], zone after zone, into ids_out[sum h]
extern "C" int da_debug_zoned_ids(const int32_t *h, int zones, int64_t M, int64_t *ids_out) {
  if (!h || !ids_out || zones < 1 || zones > ES_ZONES || M < 0) return fail(DA_ERR_BAD_ARG, "zoned ids: bad arguments");
  for (int z = 0; z < zones; ++z)
    for (int64_t q = 0; q < h[z]; ++q) *ids_out++ = M + zoned_rank(h, zones, z, q);
  return DA_OK;
}
// tests: the hash that picks a string's start slot in the duplicate plan's table (da_common.hpp dd_hash), on the host
extern "C" int da_debug_dd_hash(const uint8_t *bytes, int32_t len, uint32_t *out) {
  if (!out || len < 0 || (len > 0 && !bytes)) return fail(DA_ERR_BAD_ARG, "dd hash: bad arguments");
  *out = dd_hash(bytes, 0, len);
  return DA_OK;
}
// tests: the sorted order the ordered DP's prefix sharing uses (launch_nw_sort_unique) on n strings of residue CODES: perm[n] and lcp[n] copied to
// d_perm_out / d_lcp_out.  Allocates the sort's workspace; synchronises `stream`.
extern "C" int da_debug_nw_sort_unique(const uint8_t *d_codes, const int64_t *d_off, int64_t n, int32_t *d_perm_out, uint8_t *d_lcp_out, void *stream) {
  if (!d_codes || !d_off || !d_perm_out || !d_lcp_out || n < 1 || n > 0x7ffffff0LL) return fail(DA_ERR_BAD_ARG, "nw sort: bad arguments");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  DevBuf work;
  const size_t sb = nw_sort_unique_workspace_bytes(n);
  const int32_t *perm = nullptr;
  const uint8_t *lcp = nullptr;
  int rc;
  if ((rc = work.alloc(sb)) != DA_OK) return rc;
  if ((rc = launch_nw_sort_unique(d_codes, d_off, n, work.p, sb, &perm, &lcp, st)) != DA_OK) return rc;
  DA_HIP_TRY(hipMemcpyAsync(d_perm_out, perm, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
  DA_HIP_TRY(hipMemcpyAsync(d_lcp_out, lcp, (size_t)n, hipMemcpyDeviceToDevice, st));
  DA_HIP_TRY(hipStreamSynchronize(st));                     // the workspace goes back to the cache after this
  return DA_OK;
}

// tests: whether the calling thread's last similarityMH call kept its count table packed (9 bits per count; the row forms with n_hash <= 511)
extern "C" int da_debug_mh_last_table_packed(int *packed_out) {
  if (!packed_out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  *packed_out = mh_route().packed_table ? 1 : 0;
  return DA_OK;
}

int da_mh_last_route(int64_t *n_out, int64_t *unique_out, int *dedup_taken_out, int *plane_bits_out, double *ms6_out) {
  const MhRoute &r = mh_route();
  if (n_out) *n_out = r.n;
  if (unique_out) *unique_out = r.unique;
  if (dedup_taken_out) *dedup_taken_out = r.taken;
  if (plane_bits_out) *plane_bits_out = r.plane_bits;
  if (ms6_out) for (int i = 0; i < 6; ++i) ms6_out[i] = r.ms[i];
  return DA_OK;
}

// ---- two sets: x (m sequences) against y (n sequences), the m x n rectangle ------------------------------------------------------------------
int da_dev_mh_compare_rect(const uint32_t *d_planes, int plane_bits, int64_t n, int n_hash, int64_t row_begin, int64_t row_end, int64_t col_begin,
                           int64_t col_end, int kind, void *d_out, int64_t ld, void *stream) {
  if (n <= 0) return fail(DA_ERR_EMPTY_INPUT, "%s", da_status_message(DA_ERR_EMPTY_INPUT));
  if (n_hash <= 0) return fail(DA_ERR_BAD_NHASH, "%s", da_status_message(DA_ERR_BAD_NHASH));
  if (!d_planes || !d_out) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (row_begin < 0 || row_end > n || row_begin > row_end) return fail(DA_ERR_BAD_ARG, "bad row range");
  if (col_begin < 0 || col_end > n || col_begin > col_end) return fail(DA_ERR_BAD_ARG, "bad column range");
  if (ld < col_end - col_begin) return fail(DA_ERR_BAD_ARG, "ld (%lld) < columns (%lld)", (long long)ld, (long long)(col_end - col_begin));
  if (kind != DA_OUT_F64 && kind != DA_OUT_COMPACT) return fail(DA_ERR_BAD_ARG, "bad output kind");
  if (n_hash > 65535)
    return fail(DA_ERR_UNSUPPORTED, "the compare kernel counts in 16 bits: n_hash <= 65535 (got %d)", n_hash);
  if (reinterpret_cast<uintptr_t>(d_planes) & 15) return fail(DA_ERR_BAD_ARG, "bit-plane buffer must be 16-byte aligned");
  if (plane_bits != 8 && plane_bits != 12 && plane_bits != 14 && plane_bits != 15 && plane_bits != 16 && plane_bits != 32)
    return fail(DA_ERR_BAD_ARG, "plane_bits must be 8, 12, 14, 15, 16 or 32 (got %d)", plane_bits);
  return launch_mh_compare_rect(d_planes, n, n_hash, row_begin, row_end, col_begin, col_end, kind, d_out, ld, static_cast<hipStream_t>(stream),
                                plane_bits);
}

namespace {
// The compare operand of two sets: ONE signature matrix [x ; filler ; y] -- x padded to a multiple of 128 rows, so that both origins of the
// rectangle are tile-aligned in the operand and the hand-scheduled loops take its interior -- and K1b ONCE on all of it: a cross pair is never on
// the diagonal, so two strings agree only through codes of the same column dictionaries.  The filler rows repeat real rows (every equality is
// kept) and their results are never stored.  The rectangle is rows [0, m) x columns [m_pad, m_pad + n) of the `rows`-row problem.
struct MhCrossOperand {
  DevBuf sig, planes, work;
  int64_t m = 0, m_pad = 0, n = 0, rows = 0;
  int bits = 32;
};
int mh_cross_operand(const uint8_t *d_xres, const int64_t *d_xoff, int64_t m, const uint8_t *d_yres, const int64_t *d_yoff, int64_t n, int k,
                     int n_hash, const uint32_t *d_seeds, MhCrossOperand *c, hipStream_t stream) {
  int rc;
  const int64_t lds = sig_ld_for(n_hash);
  c->m = m; c->n = n;
  c->m_pad = (m + 127) / 128 * 128;
  if (c->m_pad + n > DA_DICT_MAX_N && m + n <= DA_DICT_MAX_N) c->m_pad = m;   // keep the dictionary rather than the alignment
  const int64_t rows = c->rows = c->m_pad + n;
  const size_t wb = mh_planes_workspace_bytes(rows, n_hash);
  if ((rc = c->sig.alloc((size_t)rows * lds * sizeof(uint32_t))) != DA_OK ||
      (rc = c->planes.alloc((size_t)mh_planes_words(rows, n_hash) * sizeof(uint32_t))) != DA_OK || (rc = c->work.alloc(wb)) != DA_OK) return rc;
  uint32_t *sig = c->sig.as<uint32_t>();
  if ((rc = launch_minhash_signatures(d_xres, d_xoff, m, k, n_hash, d_seeds, sig, lds, stream)) != DA_OK ||
      (rc = launch_minhash_signatures(d_yres, d_yoff, n, k, n_hash, d_seeds, sig + c->m_pad * lds, lds, stream)) != DA_OK ||
      (rc = launch_fill_sig_rows(sig, lds, m, c->m_pad, n_hash, stream)) != DA_OK) return rc;
  return build_planes(sig, lds, rows, n_hash, 0, c->work.p, wb, c->planes.as<uint32_t>(), &c->bits, stream);
}
int mh_cross_compare(const MhCrossOperand &c, int n_hash, int64_t r0, int64_t r1, int kind, void *d_out, int64_t ld, hipStream_t stream) {
  return launch_mh_compare_rect(c.planes.as<uint32_t>(), c.rows, n_hash, r0, r1, c.m_pad, c.m_pad + c.n, kind, d_out, ld, stream, c.bits);
}
struct MhCrossRoute { int64_t m = 0, n = 0, ux = 0, uy = 0; int taken = 0, plane_bits = 0; float ms[5] = {0, 0, 0, 0, 0}; };   // plan, K1 + K1b, K2, copy lists, expansion
static MhCrossRoute &mh_cross_route() { static thread_local MhCrossRoute r; return r; }
struct CrossEvents {
  hipEvent_t e[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  ~CrossEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};
// one side's duplicate plan (byte-identical strings collapsed): the unique count, and -- built on demand -- ids, unique strings, offsets
struct CrossSide { DevBuf work; NwDedupPlan p{}; int64_t U = 0; };
}  // namespace

// similarityMH_cross on two resident sets as ONE call: direct (K1 per side, K1b on the union, the rectangle compare into d_out) or, when
// collapsing byte-identical strings PER SIDE shrinks the compare enough, the rectangular duplicate route: the U_x x U_y count table of the unique
// strings, then the rectangular row expansion (launch_expand_stream_rect).  One stream, no pipelining, no packed table, no heavy / rare split,
// no sparse route.
int da_dev_similarity_mh_cross(const uint8_t *d_x_residues, const int64_t *d_x_offsets, int64_t m, int64_t x_total, const uint8_t *d_y_residues,
                               const int64_t *d_y_offsets, int64_t n, int64_t y_total, int k, int n_hash, const uint32_t *d_seeds, double *d_out,
                               int64_t ld, void *stream_v) {
  int rc;
  if ((rc = validate_mh(m, k > 0 ? k : 1, n_hash > 0 ? n_hash : 1)) != DA_OK || (rc = validate_mh(n, k, n_hash)) != DA_OK) return rc;   // x empty, y empty, k, n_hash
  if (!d_x_residues || !d_x_offsets || !d_y_residues || !d_y_offsets || !d_seeds || !d_out) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (ld < n) return fail(DA_ERR_BAD_ARG, "ld (%lld) < n (%lld)", (long long)ld, (long long)n);
  if (n_hash > 65535) return fail(DA_ERR_UNSUPPORTED, "the compare kernel counts in 16 bits: the two-set calls take n_hash <= 65535 (got %d)", n_hash);
  if (m > 0x7ffffff0LL || n > 0x7ffffff0LL) return fail(DA_ERR_UNSUPPORTED, "two-set MinHash: too many sequences");
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  const Config &cfg = da::config();
  MhCrossRoute &route = mh_cross_route() = MhCrossRoute();
  route.m = m; route.n = n; route.ux = m; route.uy = n;
  CrossEvents ev;
  for (auto &e : ev.e) DA_HIP_TRY(hipEventCreate(&e));
  DA_HIP_TRY(hipEventRecord(ev.e[0], stream));
  // admission of the duplicate route: the compare shrinks by U_x U_y / (m n) and the expansion costs what the direct kernel's stores cost, so --
  // like the square route's U / n <= 0.68 -- it pays while sqrt(U_x U_y / (m n)) stays below that share (DYNAALIGN_MH_DEDUP_MAX_PCT changes
  // it, DYNAALIGN_MH_DEDUP_MIN_N is compared with m + n)
  CrossSide sx, sy;
  bool take = false;
  const int64_t min_n = cfg.mh_dedup_min_n >= 0 ? cfg.mh_dedup_min_n : 2048;
  if (!cfg.mh_no_dedup && m + n >= min_n && x_total > 0 && y_total > 0 && n_hash <= 2047) {
    if ((rc = mh_count_unique(d_x_residues, d_x_offsets, m, x_total, &sx.work, &sx.p, &sx.U, stream)) != DA_OK ||
        (rc = mh_count_unique(d_y_residues, d_y_offsets, n, y_total, &sy.work, &sy.p, &sy.U, stream)) != DA_OK) return rc;
    route.ux = sx.U; route.uy = sy.U;
    const double pct = (double)(cfg.mh_dedup_max_pct >= 0 ? cfg.mh_dedup_max_pct : 68);
    take = sx.U > 0 && sy.U > 0 && (double)sx.U * (double)sy.U * 10000.0 <= (double)m * (double)n * pct * pct &&
           expand_stream_rect_ok(m, n, sx.U, sy.U, n_hash, d_out, ld);
    if (take && ((rc = launch_nw_dedup_build(d_x_residues, d_x_offsets, m, sx.U, sx.p, stream, DedupOrder::first)) != DA_OK ||
                 (rc = launch_nw_dedup_build(d_y_residues, d_y_offsets, n, sy.U, sy.p, stream, DedupOrder::first)) != DA_OK)) return rc;
  }
  DA_HIP_TRY(hipEventRecord(ev.e[1], stream));
  MhCrossOperand c;
  if ((rc = take ? mh_cross_operand(sx.p.ucodes, sx.p.uoff, sx.U, sy.p.ucodes, sy.p.uoff, sy.U, k, n_hash, d_seeds, &c, stream)
                 : mh_cross_operand(d_x_residues, d_x_offsets, m, d_y_residues, d_y_offsets, n, k, n_hash, d_seeds, &c, stream)) != DA_OK) return rc;
  route.plane_bits = c.bits;
  DA_HIP_TRY(hipEventRecord(ev.e[2], stream));
  DevBuf dtab, ex;
  if (!take) {
    if ((rc = mh_cross_compare(c, n_hash, 0, m, DA_OUT_F64, d_out, ld, stream)) != DA_OK) return rc;
    DA_HIP_TRY(hipEventRecord(ev.e[3], stream));
  } else {
    const int64_t ld_d = (sy.U + 7) / 8 * 8;
    if ((rc = dtab.alloc((size_t)sx.U * (size_t)ld_d * 2)) != DA_OK || (rc = ex.alloc(expand_stream_scratch_bytes(m, sx.U))) != DA_OK) return rc;
    if ((rc = mh_cross_compare(c, n_hash, 0, sx.U, DA_OUT_COMPACT, dtab.p, ld_d, stream)) != DA_OK) return rc;
    DA_HIP_TRY(hipEventRecord(ev.e[3], stream));
    if ((rc = launch_expand_stream_rect(dtab.as<uint16_t>(), ld_d, sx.p.uidx, m, sx.U, sy.p.uidx, n, sy.U, n_hash, d_out, ld, ex.p, stream,
                                        ev.e[4])) != DA_OK) return rc;
    DA_HIP_TRY(hipEventRecord(ev.e[5], stream));
  }
  DA_HIP_TRY(hipStreamSynchronize(stream));            // the intermediates go back to the cache after this
  route.taken = take ? 1 : 0;
  for (int i = 0; i < (take ? 5 : 3); ++i) (void)hipEventElapsedTime(&route.ms[i], ev.e[i], ev.e[i + 1]);
  return DA_OK;
}

int da_mh_cross_last_route(int64_t *m_out, int64_t *n_out, int64_t *unique_x_out, int64_t *unique_y_out, int *route_out, int *plane_bits_out,
                           double *ms5_out) {
  const MhCrossRoute &r = mh_cross_route();
  if (m_out) *m_out = r.m;
  if (n_out) *n_out = r.n;
  if (unique_x_out) *unique_x_out = r.ux;
  if (unique_y_out) *unique_y_out = r.uy;
  if (route_out) *route_out = r.taken;
  if (plane_bits_out) *plane_bits_out = r.plane_bits;
  if (ms5_out) for (int i = 0; i < 5; ++i) ms5_out[i] = r.ms[i];
  return DA_OK;
}

// ---- two sets, top-k per row: the rectangle as uint16 codes in row blocks, the selection kernel on each block ------------------------------
int da_dev_topk_rows(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, const uint16_t *d_rank, int rank_bits, int top, int32_t *d_idx,
                     uint16_t *d_key_out, int64_t ld_out, void *stream) {
  if (rows < 0 || n < 0) return fail(DA_ERR_BAD_ARG, "negative shape");
  if (rows == 0) return DA_OK;
  if (!d_keys || !d_idx || !d_key_out) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (ld < n) return fail(DA_ERR_BAD_ARG, "ld (%lld) < n (%lld)", (long long)ld, (long long)n);
  if (rank_bits < 0 || rank_bits > 16) return fail(DA_ERR_BAD_ARG, "rank_bits must be 0 .. 16 (got %d)", rank_bits);
  if (top >= 1 && top <= n && top <= DA_TOPK_MAX && ld_out < top) return fail(DA_ERR_BAD_ARG, "ld_out (%lld) < top (%d)", (long long)ld_out, top);
  return launch_topk_rows(d_keys, rows, n, ld, d_rank, rank_bits, top, d_idx, ld_out, d_key_out, ld_out, static_cast<hipStream_t>(stream));
}

// the same selection with every row's own column left out: row r of the block owns column self_col0 + r (dynaalign.h)
int da_dev_topk_rows_self(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, const uint16_t *d_rank, int rank_bits, int top, int64_t self_col0,
                          int32_t *d_idx, uint16_t *d_key_out, int64_t ld_out, uint16_t *d_self_key, void *stream) {
  if (rows < 0 || n < 0) return fail(DA_ERR_BAD_ARG, "negative shape");
  if (rows == 0) return DA_OK;
  if (!d_keys || !d_idx || !d_key_out) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (ld < n) return fail(DA_ERR_BAD_ARG, "ld (%lld) < n (%lld)", (long long)ld, (long long)n);
  if (rank_bits < 0 || rank_bits > 16) return fail(DA_ERR_BAD_ARG, "rank_bits must be 0 .. 16 (got %d)", rank_bits);
  if (top >= 1 && top <= n - 1 && top <= DA_TOPK_MAX && ld_out < top) return fail(DA_ERR_BAD_ARG, "ld_out (%lld) < top (%d)", (long long)ld_out, top);
  return launch_topk_rows_self(d_keys, rows, n, ld, d_rank, rank_bits, top, self_col0, d_idx, ld_out, d_key_out, ld_out, d_self_key,
                               static_cast<hipStream_t>(stream));
}

namespace {
// 1 <= top <= n (DA_ERR_BAD_ARG), top <= DA_TOPK_MAX (DA_ERR_UNSUPPORTED): what every top-k entry point says after its own validation
int topk_check(int top, int64_t n) {
  if (top < 1 || top > n) return fail(DA_ERR_BAD_ARG, "top must be in 1 .. n (got top = %d, n = %lld)", top, (long long)n);
  if (top > DA_TOPK_MAX)
    return fail(DA_ERR_UNSUPPORTED, "top-k per row keeps its candidates in a fixed LDS buffer: top <= %d (got %d)", DA_TOPK_MAX, top);
  return DA_OK;
}
// the one-set lists: a second sequence, 1 <= top <= n - 1 (DA_ERR_BAD_ARG), top <= DA_TOPK_MAX (DA_ERR_UNSUPPORTED, topk_check's text)
int knn_check(int top, int64_t n) {
  if (n < 2) return fail(DA_ERR_BAD_ARG, "a nearest neighbour needs a second sequence");
  if (top < 1 || top > n - 1) return fail(DA_ERR_BAD_ARG, "top must be in 1 .. n - 1 (got top = %d, n = %lld)", top, (long long)n);
  if (top > DA_TOPK_MAX)
    return fail(DA_ERR_UNSUPPORTED, "top-k per row keeps its candidates in a fixed LDS buffer: top <= %d (got %d)", DA_TOPK_MAX, top);
  return DA_OK;
}
int bits_of(int64_t max_value) {
  int b = 1;
  while (b < 16 && (max_value >> b) != 0) ++b;
  return b;
}
// Rows [0, m) of a two-set rectangle with n columns, selected block by block: compute(b0, b1, d, ld) writes the uint16 codes of rows [b0, b1)
// to the scratch block d (leading dimension ld: n rounded up to a multiple of 8, so that rows are read in 16-byte units), then
// da_dev_topk_rows' kernel takes `top` of every row into d_idx / d_key.  The block is sized like rows_to_host's: by the column count alone.
// Synchronises the stream (the scratch block goes back to the cache).  self: the rectangle is the square problem's own rows (m == n, columns
// [0, n)), so the block starting at row b0 runs the self form of the selection with self_col0 = b0; d_self_key (may be NULL) receives the diagonal keys.
int topk_blocks(int64_t m, int64_t n, const uint16_t *d_rank, int rank_bits, int top, int32_t *d_idx, int64_t ld_idx, uint16_t *d_key,
                int64_t ld_key, hipStream_t stream, const std::function<int(int64_t, int64_t, void *, int64_t)> &compute, bool self = false,
                uint16_t *d_self_key = nullptr) {
  const int64_t ld = (n + 7) / 8 * 8;
  const int64_t blk = std::min(block_rows(ld, sizeof(uint16_t)), m);
  DevBuf d;
  int rc;
  if ((rc = d.alloc((size_t)blk * (size_t)ld * sizeof(uint16_t))) != DA_OK) return rc;
  for (int64_t b0 = 0; b0 < m; b0 += blk) {
    const int64_t b1 = std::min(m, b0 + blk);
    if ((rc = compute(b0, b1, d.p, ld)) != DA_OK) return rc;
    rc = self ? launch_topk_rows_self(d.as<uint16_t>(), b1 - b0, n, ld, d_rank, rank_bits, top, b0, d_idx + b0 * ld_idx, ld_idx, d_key + b0 * ld_key,
                                      ld_key, d_self_key ? d_self_key + b0 : nullptr, stream)
              : launch_topk_rows(d.as<uint16_t>(), b1 - b0, n, ld, d_rank, rank_bits, top, d_idx + b0 * ld_idx, ld_idx, d_key + b0 * ld_key, ld_key, stream);
    if (rc != DA_OK) return rc;
  }
  DA_HIP_TRY(hipStreamSynchronize(stream));
  return DA_OK;
}
// The nearest-neighbour lists of ONE resident set: K1 once on its n sequences, the planes once (no joint operand, no padding rows), then the
// rows [b0, b1) x columns [0, n) of the square problem block by block through the self form of the selection.
int mh_knn_lists(const uint8_t *d_res, const int64_t *d_off, int64_t n, int k, int n_hash, const uint32_t *d_seeds, int top, int32_t *d_idx,
                 int64_t ld_idx, uint16_t *d_key, int64_t ld_key, hipStream_t stream) {
  int rc, bits = 32;
  const int64_t lds = sig_ld_for(n_hash);
  const size_t wb = mh_planes_workspace_bytes(n, n_hash);
  DevBuf sig, planes, work;
  if ((rc = sig.alloc((size_t)n * lds * sizeof(uint32_t))) != DA_OK ||
      (rc = planes.alloc((size_t)mh_planes_words(n, n_hash) * sizeof(uint32_t))) != DA_OK || (rc = work.alloc(wb)) != DA_OK) return rc;
  if ((rc = launch_minhash_signatures(d_res, d_off, n, k, n_hash, d_seeds, sig.as<uint32_t>(), lds, stream)) != DA_OK ||
      (rc = build_planes(sig.as<uint32_t>(), lds, n, n_hash, 0, work.p, wb, planes.as<uint32_t>(), &bits, stream)) != DA_OK) return rc;
  DA_HIP_TRY(hipStreamSynchronize(stream));
  work.release(); sig.release();                         // before the scratch block is sized
  return topk_blocks(n, n, nullptr, bits_of(n_hash), top, d_idx, ld_idx, d_key, ld_key, stream, [&](int64_t b0, int64_t b1, void *d, int64_t ld) {
    return launch_mh_compare_rect(planes.as<uint32_t>(), n, n_hash, b0, b1, 0, n, DA_OUT_COMPACT, d, ld, stream, bits);
  }, true);
}
int mh_cross_topk(MhCrossOperand &c, int n_hash, int top, int32_t *d_idx, int64_t ld_idx, uint16_t *d_key, int64_t ld_key, hipStream_t stream) {
  DA_HIP_TRY(hipStreamSynchronize(stream));
  c.work.release(); c.sig.release();                     // before the scratch block is sized
  return topk_blocks(c.m, c.n, nullptr, bits_of(n_hash), top, d_idx, ld_idx, d_key, ld_key, stream, [&](int64_t b0, int64_t b1, void *d, int64_t ld) {
    return mh_cross_compare(c, n_hash, b0, b1, DA_OUT_COMPACT, d, ld, stream);
  });
}
}  // namespace

int da_dev_similarity_mh_cross_topk(const uint8_t *d_x_residues, const int64_t *d_x_offsets, int64_t m, const uint8_t *d_y_residues,
                                    const int64_t *d_y_offsets, int64_t n, int k, int n_hash, const uint32_t *d_seeds, int top, int32_t *d_idx,
                                    double *d_val, int64_t ld_out, void *stream_v) {
  int rc;
  if ((rc = validate_mh(m, k > 0 ? k : 1, n_hash > 0 ? n_hash : 1)) != DA_OK || (rc = validate_mh(n, k, n_hash)) != DA_OK) return rc;   // x empty, y empty, k, n_hash
  if (!d_x_residues || !d_x_offsets || !d_y_residues || !d_y_offsets || !d_seeds || !d_idx || !d_val) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (n_hash > 65535) return fail(DA_ERR_UNSUPPORTED, "the compare kernel counts in 16 bits: the two-set calls take n_hash <= 65535 (got %d)", n_hash);
  if (m > 0x7ffffff0LL || n > 0x7ffffff0LL) return fail(DA_ERR_UNSUPPORTED, "two-set MinHash: too many sequences");
  if ((rc = topk_check(top, n)) != DA_OK) return rc;
  if (ld_out < top) return fail(DA_ERR_BAD_ARG, "ld_out (%lld) < top (%d)", (long long)ld_out, top);
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  MhCrossOperand c;
  DevBuf key;
  if ((rc = mh_cross_operand(d_x_residues, d_x_offsets, m, d_y_residues, d_y_offsets, n, k, n_hash, d_seeds, &c, stream)) != DA_OK) return rc;
  if ((rc = key.alloc((size_t)m * (size_t)top * sizeof(uint16_t))) != DA_OK) return rc;
  if ((rc = mh_cross_topk(c, n_hash, top, d_idx, ld_out, key.as<uint16_t>(), top, stream)) != DA_OK) return rc;
  if ((rc = launch_topk_values(key.as<uint16_t>(), top, m, top, n_hash, d_val, ld_out, stream)) != DA_OK) return rc;
  DA_HIP_TRY(hipStreamSynchronize(stream));              // the key block goes back to the cache after this
  return DA_OK;
}

// ---- one set against itself: every sequence's `top` nearest other sequences, and the graph those lists define ---------------------------------
int da_dev_similarity_mh_knn(const uint8_t *d_residues, const int64_t *d_offsets, int64_t n, int k, int n_hash, const uint32_t *d_seeds, int top,
                             int32_t *d_idx, double *d_val, int64_t ld_out, void *stream_v) {
  int rc;
  if ((rc = validate_mh(n, k, n_hash)) != DA_OK) return rc;
  if (!d_residues || !d_offsets || !d_seeds || !d_idx || !d_val) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if ((rc = knn_check(top, n)) != DA_OK) return rc;
  if (n_hash > 65535) return fail(DA_ERR_UNSUPPORTED, "the compare kernel counts in 16 bits: n_hash <= 65535 (got %d)", n_hash);
  if (n > 0x7ffffff0LL) return fail(DA_ERR_UNSUPPORTED, "nearest-neighbour lists: too many sequences");
  if (ld_out < top) return fail(DA_ERR_BAD_ARG, "ld_out (%lld) < top (%d)", (long long)ld_out, top);
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  DevBuf key;
  if ((rc = key.alloc((size_t)n * (size_t)top * sizeof(uint16_t))) != DA_OK) return rc;
  if ((rc = mh_knn_lists(d_residues, d_offsets, n, k, n_hash, d_seeds, top, d_idx, ld_out, key.as<uint16_t>(), top, stream)) != DA_OK) return rc;
  if ((rc = launch_topk_values(key.as<uint16_t>(), top, n, top, n_hash, d_val, ld_out, stream)) != DA_OK) return rc;
  DA_HIP_TRY(hipStreamSynchronize(stream));              // the key block goes back to the cache after this
  return DA_OK;
}

size_t da_dev_knn_edges_bytes(int64_t n, int top) { return knn_edges_workspace_bytes(n, top); }

int da_dev_knn_edges(const int32_t *d_idx, const uint16_t *d_key, int64_t ld, int64_t n, int top, int mode, int is_nw, const uint16_t *d_self_key,
                     int self_code, int loops, void *d_work, size_t work_bytes, int32_t *d_i, int32_t *d_j, uint16_t *d_v, uint64_t *d_count,
                     void *stream) {
  if (n <= 0) return fail(DA_ERR_EMPTY_INPUT, "%s", da_status_message(DA_ERR_EMPTY_INPUT));
  if (top < 1 || top > DA_TOPK_MAX) return fail(DA_ERR_BAD_ARG, "top must be in 1 .. %d (got %d)", DA_TOPK_MAX, top);
  if (ld < top) return fail(DA_ERR_BAD_ARG, "ld (%lld) < top (%d)", (long long)ld, top);
  if (mode != DA_KNN_UNION && mode != DA_KNN_MUTUAL) return fail(DA_ERR_BAD_ARG, "mode must be DA_KNN_UNION or DA_KNN_MUTUAL (got %d)", mode);
  if (self_code < 0 || self_code > 65535) return fail(DA_ERR_BAD_ARG, "self_code must be a uint16 code (got %d)", self_code);
  if (!d_idx || !d_key || !d_work || !d_i || !d_j || !d_v || !d_count) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (reinterpret_cast<uintptr_t>(d_work) & 255) return fail(DA_ERR_BAD_ARG, "workspace must be 256-byte aligned");
  return launch_knn_edges(d_idx, d_key, ld, n, top, mode == DA_KNN_MUTUAL, is_nw != 0, d_self_key, self_code, loops != 0, d_work, work_bytes, d_i, d_j,
                          d_v, d_count, static_cast<hipStream_t>(stream));
}

// ---- pieces of the duplicate-collapsing routes for callers that orchestrate the steps themselves (the one-process-per-GPU
// sharded drivers in dynaalign_amd/sharding.py: every rank builds the same plan, computes ITS shard of the unique table,
// all-gathers the shards -- 0.2x the bytes of the N x N shards at N = 100k -- and expands locally)
size_t da_dev_unique_plan_bytes(int64_t n, int64_t total_bytes) {
  if (n <= 0) return 256;
  return nw_dedup_workspace_bytes(n, total_bytes > 0 ? total_bytes : 1);
}

int da_dev_unique_plan(const uint8_t *d_bytes, const int64_t *d_offsets, int64_t n, int64_t total_bytes, void *d_work, size_t work_bytes,
                       da_unique_plan *plan, void *stream_v) {
  if (!plan || plan->struct_size < sizeof(da_unique_plan)) return fail(DA_ERR_BAD_ARG, "da_unique_plan: NULL or struct_size too small");
  if (n <= 0) return fail(DA_ERR_EMPTY_INPUT, "%s", da_status_message(DA_ERR_EMPTY_INPUT));
  if (n > 0x7ffffff0LL) return fail(DA_ERR_UNSUPPORTED, "unique plan: n too large");
  if (!d_bytes || !d_offsets || !d_work) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if ((reinterpret_cast<uintptr_t>(d_work) & 255) || work_bytes < da_dev_unique_plan_bytes(n, total_bytes))
    return fail(DA_ERR_BAD_ARG, "workspace must be 256-byte aligned and hold da_dev_unique_plan_bytes(n, total_bytes) bytes");
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  int rc;
  const NwDedupPlan p = nw_dedup_layout(d_work, n, total_bytes > 0 ? total_bytes : 1);
  int64_t U = 0;
  if ((rc = count_unique(d_bytes, d_offsets, n, p, stream, &U)) != DA_OK) return rc;
  if (U <= 0 || U > n) return fail(DA_ERR_HIP, "unique plan: inconsistent counts (%lld unique of %lld)", (long long)U, (long long)n);
  if ((rc = launch_nw_dedup_build(d_bytes, d_offsets, n, U, p, stream)) != DA_OK) return rc;
  plan->n = n; plan->unique = U;
  plan->d_uidx = p.uidx; plan->d_ufirst = p.ufirst; plan->d_ulast = p.ulast;
  plan->d_ubytes = p.ucodes; plan->d_uoffsets = p.uoff;
  plan->d_minfirst = p.minfirst; plan->d_maxlast = p.maxlast;
  return DA_OK;
}

int da_dev_shards_to_table(const void *d_gathered, int64_t ld_g, int64_t n, int world, int value_bits, uint16_t *d_table, int64_t ld_table,
                           void *stream) {
  if (n <= 0) return fail(DA_ERR_EMPTY_INPUT, "%s", da_status_message(DA_ERR_EMPTY_INPUT));
  if (!d_gathered || !d_table) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (world < 1 || ld_table < n) return fail(DA_ERR_BAD_ARG, "bad world / leading dimension");
  if (value_bits != 0 && (value_bits < 1 || value_bits > 16)) return fail(DA_ERR_BAD_ARG, "value_bits must be 0 (uint16 blocks) or 1..16");
  const ShardGeom g = shard_geom(n, world, 128);
  if (value_bits == 0 && ld_g < g.W) return fail(DA_ERR_BAD_ARG, "ld_g (%lld) < da_shard_ld (%lld)", (long long)ld_g, (long long)g.W);
  return launch_shards_to_table(d_gathered, ld_g, g, value_bits, d_table, ld_table, static_cast<hipStream_t>(stream));
}

size_t da_dev_expand_workspace_bytes(int64_t n, int64_t unique, int is_nw, int n_hash, int nw_max_len) {
  const size_t b = expand_rows_workspace_bytes(n, unique, DA_OUT_F64, is_nw != 0, n_hash, nw_max_len);
  return b ? b : 256;                                          // (shapes the two streaming passes do not cover use no workspace)
}

int da_dev_expand_unique(const uint16_t *d_table, int64_t ld_table, int table_world, const da_unique_plan *plan, int is_nw, int n_hash,
                         int nw_max_len, void *d_work, size_t work_bytes, double *d_out, int64_t ld, void *stream) {
  if (!plan || plan->struct_size < sizeof(da_unique_plan) || !plan->d_uidx || !plan->d_ufirst) return fail(DA_ERR_BAD_ARG, "bad da_unique_plan");
  if (!d_table || !d_out) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  const int64_t n = plan->n, U = plan->unique;
  if (n <= 0 || U <= 0 || U > n || ld < n || ld_table < U) return fail(DA_ERR_BAD_ARG, "bad sizes / leading dimensions");
  if (!is_nw && (n_hash <= 0 || n_hash > 65535)) return fail(DA_ERR_BAD_NHASH, "%s", da_status_message(DA_ERR_BAD_NHASH));
  if (table_world < 1) return fail(DA_ERR_BAD_ARG, "table_world must be >= 1");
  const int64_t rows_local = table_world > 1 ? ceil_div(ceil_div(U, 128), table_world) * 128 : 0;
  // MinHash (symmetric table, one block): the ROW expansion -- every output row written once from its table row in LDS, no gathered copy
  // (minhash_kernels.hip k_expand_stream; DYNAALIGN_EXPAND_NO_STREAM=1 keeps the tile passes).  The copy lists live in the caller's workspace.
  if (!is_nw && table_world == 1 && expand_stream_ok(n, U, n_hash, d_out, ld) && (ld_table & 7) == 0 && ld_table <= 65536 &&
      (reinterpret_cast<uintptr_t>(d_table) & 15) == 0) {
    const size_t lists_bytes = expand_stream_scratch_bytes(n, U);
    if (d_work && work_bytes >= lists_bytes && (reinterpret_cast<uintptr_t>(d_work) & 15) == 0)
      return launch_expand_stream(d_table, ld_table, plan->d_uidx, n, U, n_hash, d_out, ld, d_work, static_cast<hipStream_t>(stream));
    DevBuf lists;
    int rc = lists.alloc(lists_bytes);
    if (rc != DA_OK) return rc;
    rc = launch_expand_stream(d_table, ld_table, plan->d_uidx, n, U, n_hash, d_out, ld, lists.p, static_cast<hipStream_t>(stream));
    DA_HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));   // the lists go away with this frame
    return rc;
  }
  const size_t need = expand_rows_workspace_bytes(n, U, DA_OUT_F64, is_nw != 0, n_hash, nw_max_len);
  uint16_t *d_F = (need && d_work && work_bytes >= need && (reinterpret_cast<uintptr_t>(d_work) & 15) == 0) ? static_cast<uint16_t *>(d_work) : nullptr;
  if ((ld_table & 7) || (reinterpret_cast<uintptr_t>(d_table) & 15)) d_F = nullptr;     // the column gather reads the table in 16-byte units
  return launch_expand_unique(d_table, ld_table, plan->d_uidx, n, DA_OUT_F64, is_nw != 0, n_hash, d_out, ld, static_cast<hipStream_t>(stream),
                              nw_max_len, d_F, plan->d_ufirst, U, nullptr, nullptr, table_world, rows_local);
}

size_t da_dev_unique_rows_bytes(int64_t n, int64_t unique) {
  if (n <= 0 || unique <= 0) return 256;
  return (size_t)unique * (size_t)(ceil_div(n, 8) * 8) * 2;
}

int da_dev_unique_rows(const uint16_t *d_table, int64_t ld_table, const da_unique_plan *plan, uint16_t *d_rows, void *stream) {
  if (!plan || plan->struct_size < sizeof(da_unique_plan) || !plan->d_uidx || !plan->d_ufirst) return fail(DA_ERR_BAD_ARG, "bad da_unique_plan");
  if (!d_table || !d_rows) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (ld_table < plan->unique) return fail(DA_ERR_BAD_ARG, "ld_table < unique");
  return launch_gather_columns(d_table, ld_table, plan->d_uidx, plan->d_ufirst, plan->n, plan->unique, d_rows, ceil_div(plan->n, 8) * 8, true,
                               static_cast<hipStream_t>(stream));
}

int da_dev_nw_unique_rows(const da_unique_plan *plan, int64_t max_len, int matrix_id, int gap_open, int gap_ext, int rank, int world,
                          uint16_t *d_out, int64_t ld, void *stream) {
  if (!plan || plan->struct_size < sizeof(da_unique_plan) || !plan->d_ubytes || !plan->d_uoffsets || !plan->d_ufirst || !plan->d_minfirst ||
      !plan->d_maxlast)
    return fail(DA_ERR_BAD_ARG, "bad da_unique_plan");
  if (!d_out) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  const int64_t U = plan->unique;
  if (world < 1 || rank < 0 || rank >= world || ld < U) return fail(DA_ERR_BAD_ARG, "bad rank / world / leading dimension");
  if (matrix_id < 0 || matrix_id >= matrix_count_host()) return fail(DA_ERR_BAD_MATRIX, "%s", da_status_message(DA_ERR_BAD_MATRIX));
  if (max_len < 1 || max_len > 64 || gap_open < 0 || gap_ext < 0)
    return fail(DA_ERR_UNSUPPORTED, "the ordered unique-table sweep serves sequences of 1..64 residues and penalties >= 0");
  // world = 1: the whole table in natural row order; world > 1: this rank's cyclic 128-row units, stored back to back -- one launch
  return launch_nw(plan->d_ubytes, plan->d_uoffsets, U, max_len, matrix_id, gap_open, gap_ext, 0, U, false, DA_OUT_COMPACT, d_out, ld, nullptr, 0,
                   static_cast<hipStream_t>(stream), rank, world > 1 ? world : 0, plan->d_ufirst, plan->d_minfirst, plan->d_maxlast);
}

int da_dev_nw_encode(const uint8_t *d_residues, int64_t total_residues, uint8_t *d_codes,
                     int32_t *d_bad, void *stream) {
  if (total_residues > 0 && (!d_residues || !d_codes || !d_bad)) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  return launch_nw_encode(d_residues, total_residues, d_codes, d_bad, static_cast<hipStream_t>(stream));
}

// similarityNW over the WHOLE pair space (symmetric mode) with byte-identical sequences collapsed first (nw_kernels.hip:
// "duplicate sequences"): plan -> (host reads the unique count: one stream synchronisation) -> ordered DP on the unique table
// -> index expansion to the n x n result.  Exact.  Taken when at least 15 % of the sequences are duplicates; otherwise, or
// for what the route does not cover (sequences > 64 residues, out-of-range penalties, score output, 32-bit packed output,
// n < 2048), the direct kernel runs.  Synchronises `stream` before returning when the route is taken (its buffers are parked
// for the next call).  DYNAALIGN_NW_NO_DEDUP=1 switches it off.
// what the last whole-matrix NW call of this thread did (da_nw_last_route: bench.py's roofline object needs the DP
// kernel's own duration, and the call is one C entry point)
struct NwRoute { int64_t n = 0, unique = 0; int taken = 0; float plan_ms = 0, dp_ms = 0, expand_ms = 0; };
static NwRoute &nw_route() { static thread_local NwRoute r; return r; }

static int nw_full_symmetric(const uint8_t *d_codes, const int64_t *d_offsets, int64_t n, int64_t total, int64_t max_len, int mid,
                             int gap_open, int gap_ext, int kind, void *d_out, int64_t ld, hipStream_t stream, int64_t *unique_out = nullptr) {
  int rc;
  if (unique_out) *unique_out = n;
  NwRoute &route = nw_route();
  route = NwRoute();
  route.n = route.unique = n;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  struct EvGuard { hipEvent_t *e; ~EvGuard() { for (int i = 0; i < 4; ++i) if (e[i]) (void)hipEventDestroy(e[i]); } } guard{ev};
  for (auto &e : ev) DA_HIP_TRY(hipEventCreate(&e));
  DA_HIP_TRY(hipEventRecord(ev[0], stream));
  int64_t min_n = 2048;
  if (da::config().nw_dedup_min_n >= 0) min_n = da::config().nw_dedup_min_n;   // DYNAALIGN_NW_DEDUP_MIN_N: tests lower it to reach the route with tiny inputs
  const bool eligible = n >= min_n && n <= 0x7ffffff0LL && max_len <= 64 && max_len >= 1 && (kind == DA_OUT_F64 || kind == DA_OUT_COMPACT) &&
                        gap_open >= 0 && gap_ext >= 0 && !da::config().nw_no_dedup;
  if (eligible) {
    DevBuf work;
    if ((rc = work.alloc(nw_dedup_workspace_bytes(n, total))) != DA_OK) return rc;
    const NwDedupPlan p = nw_dedup_layout(work.p, n, total);
    int64_t U = 0;
    if ((rc = count_unique(d_codes, d_offsets, n, p, stream, &U)) != DA_OK) return rc;
    if (unique_out) *unique_out = U;
    route.unique = U;
    if (U > 0 && U * 100 <= n * 85) {
      if ((rc = launch_nw_dedup_build(d_codes, d_offsets, n, U, p, stream)) != DA_OK) return rc;
      const int64_t ld_d = (U + 7) / 8 * 8;
      DevBuf dtab;
      if ((rc = dtab.alloc((size_t)U * (size_t)ld_d * 2)) != DA_OK) return rc;
      // prefix sharing of the ordered DP (k_nw_short<.., PFX>): the unique strings' lexicographic order and neighbour prefixes, sequences of
      // up to 20 residues (0.1 ms; DYNAALIGN_NW_NO_PREFIX_SHARE=1: rows in id order, every row from scratch)
      DevBuf sortw;
      const int32_t *perm = nullptr;
      const uint8_t *lcp = nullptr;
      if (max_len <= 20 && !da::config().nw_no_prefix) {
        const size_t sb = nw_sort_unique_workspace_bytes(U);
        if (sortw.alloc(sb) == DA_OK) {
          if ((rc = launch_nw_sort_unique(p.ucodes, p.uoff, U, sortw.p, sb, &perm, &lcp, stream)) != DA_OK) return rc;
        } else (void)hipGetLastError();                     // (an optimisation: without its scratch the rows run in id order)
      }
      DA_HIP_TRY(hipEventRecord(ev[1], stream));
      if ((rc = launch_nw(p.ucodes, p.uoff, U, max_len, mid, gap_open, gap_ext, 0, U, false, DA_OUT_COMPACT, dtab.p, ld_d, nullptr, 0,
                          stream, 0, 0, p.ufirst, p.minfirst, p.maxlast, perm, lcp)) != DA_OK) return rc;
      DA_HIP_TRY(hipEventRecord(ev[2], stream));
      DevBuf ftab;                                        // column-gathered twin of the table for the two-pass expansion
      const size_t fbytes = expand_rows_workspace_bytes(n, U, kind, true, 0, (int)max_len);
      if (fbytes && (rc = ftab.alloc(fbytes)) != DA_OK) return rc;
      if ((rc = launch_expand_unique(dtab.as<uint16_t>(), ld_d, p.uidx, n, kind, true, 0, d_out, ld, stream, (int)max_len,
                                     fbytes ? ftab.as<uint16_t>() : nullptr, p.ufirst, U)) != DA_OK) return rc;
      DA_HIP_TRY(hipEventRecord(ev[3], stream));
      DA_HIP_TRY(hipStreamSynchronize(stream));          // work / dtab go back to the parked-buffer cache here
      route.taken = 1;
      (void)hipEventElapsedTime(&route.plan_ms, ev[0], ev[1]);
      (void)hipEventElapsedTime(&route.dp_ms, ev[1], ev[2]);
      (void)hipEventElapsedTime(&route.expand_ms, ev[2], ev[3]);
      return DA_OK;
    }
    DA_HIP_TRY(hipStreamSynchronize(stream));
  }
  DA_HIP_TRY(hipEventRecord(ev[1], stream));
  if ((rc = launch_nw(d_codes, d_offsets, n, max_len, mid, gap_open, gap_ext, 0, n, true, kind, d_out, ld, nullptr, 0, stream)) != DA_OK) return rc;
  DA_HIP_TRY(hipEventRecord(ev[2], stream));
  DA_HIP_TRY(hipEventSynchronize(ev[2]));                // (the direct route used to be asynchronous; the timing costs that)
  (void)hipEventElapsedTime(&route.plan_ms, ev[0], ev[1]);
  (void)hipEventElapsedTime(&route.dp_ms, ev[1], ev[2]);
  return DA_OK;
}

int da_nw_last_route(int64_t *n_out, int64_t *unique_out, int *dedup_taken_out, double *ms3_out) {
  const NwRoute &r = nw_route();
  if (n_out) *n_out = r.n;
  if (unique_out) *unique_out = r.unique;
  if (dedup_taken_out) *dedup_taken_out = r.taken;
  if (ms3_out) { ms3_out[0] = r.plan_ms; ms3_out[1] = r.dp_ms; ms3_out[2] = r.expand_ms; }
  return DA_OK;
}

int da_dev_nw(const uint8_t *d_codes, const int64_t *d_offsets, int64_t n, int64_t max_len,
              int matrix_id, int gap_open, int gap_ext, int64_t row_begin, int64_t row_end,
              int symmetric, int kind, void *d_out, int64_t ld, int32_t *d_score, int64_t ld_score,
              void *stream) {
  if (n <= 0) return DA_OK;
  if (!d_codes || !d_offsets || !d_out) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (row_begin < 0 || row_end > n || row_begin > row_end) return fail(DA_ERR_BAD_ARG, "bad row range");
  if (symmetric && (row_begin != 0 || row_end != n))
    return fail(DA_ERR_BAD_ARG, "symmetric mode needs the full row range");
  if (ld < n || (d_score && ld_score < n)) return fail(DA_ERR_BAD_ARG, "leading dimension < n");
  if (kind != DA_OUT_F64 && kind != DA_OUT_COMPACT && kind != DA_OUT_PACK32) return fail(DA_ERR_BAD_ARG, "bad output kind");
  if (symmetric && !d_score && kind != DA_OUT_PACK32) {   // whole pair space: duplicates are collapsed first when that pays
    int64_t total = 0;                                     // (bytes of all sequences: last offset; one small device read)
    DA_HIP_TRY(hipMemcpyAsync(&total, d_offsets + n, 8, hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
    DA_HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return nw_full_symmetric(d_codes, d_offsets, n, total, max_len, matrix_id, gap_open, gap_ext, kind, d_out, ld,
                             static_cast<hipStream_t>(stream));
  }
  return launch_nw(d_codes, d_offsets, n, max_len, matrix_id, gap_open, gap_ext, row_begin, row_end,
                   symmetric != 0, kind, d_out, ld, d_score, ld_score, static_cast<hipStream_t>(stream));
}

// rows [row_begin, row_end) x columns [col_begin, col_end) of the row-block mode above: pair (i, j) is calc(seq[min(i, j)], seq[max(i, j)])
int da_dev_nw_rect(const uint8_t *d_codes, const int64_t *d_offsets, int64_t n, int64_t max_len, int matrix_id, int gap_open, int gap_ext,
                   int64_t row_begin, int64_t row_end, int64_t col_begin, int64_t col_end, int kind, void *d_out, int64_t ld, void *stream) {
  if (n <= 0) return DA_OK;
  if (!d_codes || !d_offsets || !d_out) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (row_begin < 0 || row_end > n || row_begin > row_end) return fail(DA_ERR_BAD_ARG, "bad row range");
  if (col_begin < 0 || col_end > n || col_begin > col_end) return fail(DA_ERR_BAD_ARG, "bad column range");
  if (ld < col_end - col_begin) return fail(DA_ERR_BAD_ARG, "leading dimension < columns");
  if (kind != DA_OUT_F64 && kind != DA_OUT_COMPACT && kind != DA_OUT_PACK32) return fail(DA_ERR_BAD_ARG, "bad output kind");
  return launch_nw_rect(d_codes, d_offsets, n, max_len, matrix_id, gap_open, gap_ext, row_begin, row_end, col_begin, col_end, kind, d_out, ld,
                        static_cast<hipStream_t>(stream));
}

// ---- the exact Jaccard index of k-shingle sets, device layer (jaccard_kernels.hip) -----------------------------------------------------------
// k in 1 .. 8 and at most `limit` shingle positions (127, the _long calls 1024) in a sequence of max_len bytes; `seq` > 0 names the (1-based)
// sequence that is too long
static int jaccard_limits(int k, int64_t max_len, int64_t seq, int limit = 127) {
  if (k > 8) return fail(DA_ERR_UNSUPPORTED, "the exact Jaccard index packs a shingle into one 64-bit key: k <= 8 (got %d)", k);
  if (max_len - k + 1 > limit) {
    if (seq > 0)
      return fail(DA_ERR_UNSUPPORTED, "sequence %lld has %lld shingle positions: the exact Jaccard index takes at most %d (length - k + 1 <= %d)",
                  (long long)seq, (long long)(max_len - k + 1), limit, limit);
    return fail(DA_ERR_UNSUPPORTED, "max_len - k + 1 = %lld shingle positions: the exact Jaccard index takes at most %d", (long long)(max_len - k + 1),
                limit);
  }
  return DA_OK;
}

int64_t da_dev_jaccard_sets_ld(int64_t max_len, int k) { return jaccard_sets_ld(max_len, k); }

int da_dev_jaccard_sets(const uint8_t *d_residues, const int64_t *d_offsets, int64_t n, int64_t max_len, int k, void *d_keys, int64_t ld_keys,
                        uint8_t *d_counts, void *stream) {
  if (n <= 0) return fail(DA_ERR_EMPTY_INPUT, "%s", da_status_message(DA_ERR_EMPTY_INPUT));
  if (k <= 0) return fail(DA_ERR_BAD_K, "%s", da_status_message(DA_ERR_BAD_K));
  if (!d_residues || !d_offsets || !d_keys || !d_counts) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (max_len < 0) return fail(DA_ERR_BAD_ARG, "negative shape");
  int rc;
  if ((rc = jaccard_limits(k, max_len, 0)) != DA_OK) return rc;
  return launch_jaccard_sets(d_residues, d_offsets, n, max_len, k, d_keys, ld_keys, d_counts, static_cast<hipStream_t>(stream));
}

int da_dev_jaccard_rect(const void *d_keys, const uint8_t *d_counts, int64_t n, int64_t ld_keys, int k, int64_t row_begin, int64_t row_end,
                        int64_t col_begin, int64_t col_end, int kind, void *d_out, int64_t ld, void *stream) {
  if (k <= 0) return fail(DA_ERR_BAD_K, "%s", da_status_message(DA_ERR_BAD_K));
  if (k > 8) return jaccard_limits(k, 0, 0);
  return launch_jaccard_rect(d_keys, d_counts, n, ld_keys, k, row_begin, row_end, col_begin, col_end, kind, d_out, ld, static_cast<hipStream_t>(stream));
}

// ... for sequences of up to 1024 shingle positions (jaccard_long_kernels.hip): the checks of the short pair, in their order
int64_t da_jaccard_sets_long_ld(int64_t max_len, int k) { return jaccard_sets_long_ld(max_len, k); }

int da_dev_jaccard_sets_long(const uint8_t *d_residues, const int64_t *d_offsets, int64_t n, int64_t max_len, int k, void *d_keys, int64_t ld_keys,
                             uint16_t *d_counts, void *stream) {
  if (n <= 0) return fail(DA_ERR_EMPTY_INPUT, "%s", da_status_message(DA_ERR_EMPTY_INPUT));
  if (k <= 0) return fail(DA_ERR_BAD_K, "%s", da_status_message(DA_ERR_BAD_K));
  if (!d_residues || !d_offsets || !d_keys || !d_counts) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (max_len < 0) return fail(DA_ERR_BAD_ARG, "negative shape");
  int rc;
  if ((rc = jaccard_limits(k, max_len, 0, 1024)) != DA_OK) return rc;
  return launch_jaccard_sets_long(d_residues, d_offsets, n, max_len, k, d_keys, ld_keys, d_counts, static_cast<hipStream_t>(stream));
}

int da_dev_jaccard_rect_long(const void *d_keys, const uint16_t *d_counts, int64_t n, int64_t ld_keys, int k, int64_t row_begin, int64_t row_end,
                             int64_t col_begin, int64_t col_end, int kind, void *d_out, int64_t ld, void *stream) {
  if (k <= 0) return fail(DA_ERR_BAD_K, "%s", da_status_message(DA_ERR_BAD_K));
  if (k > 8) return jaccard_limits(k, 0, 0);
  return launch_jaccard_rect_long(d_keys, d_counts, n, ld_keys, k, row_begin, row_end, col_begin, col_end, kind, d_out, ld,
                                  static_cast<hipStream_t>(stream));
}

// ---- the Levenshtein similarity, device layer (lev_kernels.hip) ------------------------------------------------------------------------------
// `seq` > 0 names the (1-based) sequence that is too long
static int lev_limits(int64_t max_len, int64_t seq) {
  if (max_len > 127) {
    if (seq > 0)
      return fail(DA_ERR_UNSUPPORTED, "sequence %lld is %lld bytes long: the Levenshtein similarity takes sequences of at most 127 bytes", (long long)seq,
                  (long long)max_len);
    return fail(DA_ERR_UNSUPPORTED, "max_len = %lld: the Levenshtein similarity takes sequences of at most 127 bytes", (long long)max_len);
  }
  return DA_OK;
}

size_t da_dev_lev_masks_bytes(int64_t n, int64_t max_len, int n_classes) { return lev_masks_bytes(n, max_len, n_classes); }

int da_dev_lev_masks(const uint8_t *d_residues, const int64_t *d_offsets, int64_t n, int64_t max_len, const uint8_t *class_map, int n_classes,
                     void *d_masks, size_t masks_bytes, void *stream) {
  if (n <= 0) return fail(DA_ERR_EMPTY_INPUT, "%s", da_status_message(DA_ERR_EMPTY_INPUT));
  if (!d_residues || !d_offsets || !class_map || !d_masks) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  if (max_len < 0) return fail(DA_ERR_BAD_ARG, "negative shape");
  int rc;
  if ((rc = lev_limits(max_len, 0)) != DA_OK) return rc;
  return launch_lev_masks(d_residues, d_offsets, n, max_len, class_map, n_classes, d_masks, masks_bytes, static_cast<hipStream_t>(stream));
}

int da_dev_lev_rect(const void *d_masks, int64_t n, int64_t max_len, int n_classes, int64_t row_begin, int64_t row_end, int64_t col_begin,
                    int64_t col_end, int kind, void *d_out, int64_t ld, void *stream) {
  return launch_lev_rect(d_masks, n, max_len, n_classes, row_begin, row_end, col_begin, col_end, kind, d_out, ld, static_cast<hipStream_t>(stream));
}

int da_dev_symmetrize(void *d_mat, int64_t n, int64_t ld, int kind, void *stream) {
  if (!d_mat || ld < n) return fail(DA_ERR_BAD_ARG, "bad matrix / ld");
  return launch_symmetrize(d_mat, n, ld, kind, static_cast<hipStream_t>(stream));
}

int da_dev_widen(const uint16_t *d_in, double *d_out, int64_t count, int is_nw, int n_hash, void *stream) {
  if (count > 0 && (!d_in || !d_out)) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  return launch_widen(d_in, d_out, count, is_nw != 0, n_hash, static_cast<hipStream_t>(stream));
}

// ---- row-sharding over `world` ranks: rank p owns tile rows p, p+world, ... (cyclic, so
// the upper-triangular work is balanced); the unit is 128 rows for both kinds.
int64_t da_shard_rows(int64_t n, int world, int is_nw) {
  if (n <= 0 || world <= 0) return 0;
  return shard_geom(n, world, 128).rows;
}
int64_t da_shard_ld(int64_t n, int world, int is_nw) {
  if (n <= 0 || world <= 0) return 0;
  return shard_geom(n, world, 128).W;
}

int da_dev_mh_compare_shard(const uint32_t *d_planes, int plane_bits, int64_t n, int n_hash, int rank,
                            int world, uint16_t *d_local, int64_t ld, void *stream) {
  if (n <= 0) return fail(DA_ERR_EMPTY_INPUT, "%s", da_status_message(DA_ERR_EMPTY_INPUT));
  if (n_hash <= 0) return fail(DA_ERR_BAD_NHASH, "%s", da_status_message(DA_ERR_BAD_NHASH));
  if (n_hash > 65535) return fail(DA_ERR_UNSUPPORTED, "the compare kernel counts in 16 bits: n_hash <= 65535 (got %d)", n_hash);
  if (!d_planes || !d_local || world <= 0 || rank < 0 || rank >= world) return fail(DA_ERR_BAD_ARG, "bad shard arguments");
  const ShardGeom sg = shard_geom(n, world, 128);
  if (ld < sg.W) return fail(DA_ERR_BAD_ARG, "ld (%lld) < da_shard_ld (%lld)", (long long)ld, (long long)sg.W);
  if (reinterpret_cast<uintptr_t>(d_planes) & 15) return fail(DA_ERR_BAD_ARG, "bit-plane buffer must be 16-byte aligned");
  if (plane_bits != 8 && plane_bits != 12 && plane_bits != 14 && plane_bits != 15 && plane_bits != 16 && plane_bits != 32)
    return fail(DA_ERR_BAD_ARG, "plane_bits must be 8, 12, 14, 15, 16 or 32 (got %d)", plane_bits);
  if ((int64_t)rank * 128 >= n) return DA_OK;  // this rank owns no rows
  return launch_mh_compare(d_planes, n, n_hash, (int64_t)rank * 128, n, false, DA_OUT_COMPACT, d_local, ld,
                           static_cast<hipStream_t>(stream), plane_bits, world, true, sg.Q, sg.W);
}

// ---- the MH exchange in value_bits = bits(n_hash) instead of 16 bits per count
static int packed_args_ok(int64_t n, int world, int value_bits) {
  if (n <= 0 || world <= 0) return fail(DA_ERR_BAD_ARG, "bad shard arguments");
  if (value_bits < 1 || value_bits > 16) return fail(DA_ERR_BAD_ARG, "value_bits must be in [1, 16] (got %d)", value_bits);
  return DA_OK;
}
int64_t da_shard_packed_bytes(int64_t n, int world, int value_bits) {
  if (n <= 0 || world <= 0 || value_bits < 1 || value_bits > 16) return 0;
  return shard_packed_bytes(shard_geom(n, world, 128), value_bits);
}
int da_dev_pack_shard(const uint16_t *d_local, int64_t ld, int64_t n, int world, int value_bits, uint8_t *d_packed,
                      void *stream) {
  int rc = packed_args_ok(n, world, value_bits);
  if (rc != DA_OK) return rc;
  const ShardGeom sg = shard_geom(n, world, 128);
  if (!d_local || !d_packed || ld < sg.W) return fail(DA_ERR_BAD_ARG, "bad block / ld");
  if (reinterpret_cast<uintptr_t>(d_packed) & 7) return fail(DA_ERR_BAD_ARG, "packed block must be 8-byte aligned");
  return launch_pack_shard(d_local, ld, sg, value_bits, d_packed, static_cast<hipStream_t>(stream));
}
int da_dev_finalize_shards_packed(const uint8_t *d_gathered, int64_t n, int world, int value_bits, int n_hash,
                                  double *d_out, int64_t ld_out, void *stream) {
  int rc = packed_args_ok(n, world, value_bits);
  if (rc != DA_OK) return rc;
  if (!d_gathered || !d_out || ld_out < n) return fail(DA_ERR_BAD_ARG, "bad arguments");
  if (n_hash <= 0 || n_hash >= (1 << value_bits)) return fail(DA_ERR_BAD_ARG, "n_hash (%d) does not fit value_bits (%d)", n_hash, value_bits);
  return launch_finalize_packed(d_gathered, shard_geom(n, world, 128), value_bits, n_hash, d_out, ld_out,
                                static_cast<hipStream_t>(stream));
}

int da_dev_nw_shard(const uint8_t *d_codes, const int64_t *d_offsets, int64_t n, int64_t max_len, int matrix_id,
                    int gap_open, int gap_ext, int rank, int world, uint16_t *d_local, int64_t ld, void *stream) {
  if (n <= 0) return DA_OK;
  if (!d_codes || !d_offsets || !d_local || world <= 0 || rank < 0 || rank >= world)
    return fail(DA_ERR_BAD_ARG, "bad shard arguments");
  if (ld < shard_geom(n, world, 128).W) return fail(DA_ERR_BAD_ARG, "ld < da_shard_ld");
  return launch_nw(d_codes, d_offsets, n, max_len, matrix_id, gap_open, gap_ext, 0, n, false, DA_OUT_COMPACT, d_local, ld,
                   nullptr, 0, static_cast<hipStream_t>(stream), rank, world);
}

int da_dev_finalize_shards(const uint16_t *d_gathered, int64_t ld_g, int64_t n, int world, int is_nw, int n_hash,
                           double *d_out, int64_t ld_out, void *stream) {
  if (n <= 0) return DA_OK;
  if (!d_gathered || !d_out || world <= 0 || ld_out < n) return fail(DA_ERR_BAD_ARG, "bad finalize arguments");
  const ShardGeom sg = shard_geom(n, world, 128);
  if (ld_g < sg.W) return fail(DA_ERR_BAD_ARG, "ld_g < da_shard_ld");
  return launch_finalize_sharded(d_gathered, ld_g, sg, is_nw != 0, n_hash, d_out, ld_out, static_cast<hipStream_t>(stream));
}


// ---- threshold + sparsify: the step clusterbreak applies right after sim_fn -------------

int da_dev_upper_histogram(const uint16_t *d_compact, int64_t ld, int64_t n, int nbins, uint64_t *d_hist, void *stream) {
  if (n <= 0) return DA_OK;
  if (!d_compact || !d_hist || ld < n || nbins <= 0 || nbins > 65536) return fail(DA_ERR_BAD_ARG, "bad histogram arguments");
  return launch_upper_histogram(d_compact, ld, n, nbins, reinterpret_cast<unsigned long long *>(d_hist),
                                static_cast<hipStream_t>(stream));
}

// the same two steps reading the n x n count matrix THROUGH a row map (row i = row d_rowmap[i] of d_rows: da_dev_unique_rows'
// table with the plan's d_uidx) -- the duplicate rows are never materialised
int da_dev_upper_histogram_rows(const uint16_t *d_rows, int64_t ld, const int32_t *d_rowmap, int64_t n, int nbins, uint64_t *d_hist,
                                void *stream) {
  if (n <= 0) return DA_OK;
  if (!d_rows || !d_rowmap || !d_hist || ld < n || nbins <= 0 || nbins > 65536) return fail(DA_ERR_BAD_ARG, "bad histogram arguments");
  return launch_upper_histogram(d_rows, ld, n, nbins, reinterpret_cast<unsigned long long *>(d_hist), static_cast<hipStream_t>(stream), 0, 0,
                                d_rowmap);
}

int da_dev_extract_edges_rows(const uint16_t *d_rows, int64_t ld, const int32_t *d_rowmap, int64_t n, const uint8_t *d_keep, int nbins,
                              int include_diagonal, int32_t *d_i, int32_t *d_j, uint16_t *d_v, int64_t capacity, uint64_t *d_count,
                              void *stream) {
  if (n <= 0) return DA_OK;
  if (!d_rows || !d_rowmap || !d_keep || !d_i || !d_j || !d_v || !d_count || ld < n || nbins <= 0 || nbins > 65536 || capacity < 0)
    return fail(DA_ERR_BAD_ARG, "bad edge-extraction arguments");
  if (n > 0x7fffffffLL) return fail(DA_ERR_UNSUPPORTED, "edge indices are int32");
  return launch_extract_edges(d_rows, ld, n, d_keep, nbins, include_diagonal != 0, d_i, d_j, d_v, capacity,
                              reinterpret_cast<unsigned long long *>(d_count), static_cast<hipStream_t>(stream), 0, 0, d_rowmap);
}

// The same two steps on ONE RANK'S folded shard block (da_dev_mh_compare_shard output): every unordered
// pair lives on exactly one rank, so summing the ranks' histograms (an all-reduce of n_hash+1 words) gives
// the global histogram, and the ranks' edge lists are disjoint -- no N x N exchange at all.
int da_dev_shard_histogram(const uint16_t *d_local, int64_t ld, int64_t n, int rank, int world, int nbins,
                           uint64_t *d_hist, void *stream) {
  if (n <= 0) return DA_OK;
  if (!d_local || !d_hist || world <= 0 || rank < 0 || rank >= world || nbins <= 0 || nbins > 65536 ||
      ld < shard_geom(n, world, 128).W)
    return fail(DA_ERR_BAD_ARG, "bad shard histogram arguments");
  return launch_upper_histogram(d_local, ld, n, nbins, reinterpret_cast<unsigned long long *>(d_hist),
                                static_cast<hipStream_t>(stream), rank, world);
}

int da_dev_shard_extract_edges(const uint16_t *d_local, int64_t ld, int64_t n, int rank, int world,
                               const uint8_t *d_keep, int nbins, int include_diagonal, int32_t *d_i, int32_t *d_j,
                               uint16_t *d_v, int64_t capacity, uint64_t *d_count, void *stream) {
  if (n <= 0) return DA_OK;
  if (!d_local || !d_keep || !d_i || !d_j || !d_v || !d_count || world <= 0 || rank < 0 || rank >= world || nbins <= 0 ||
      nbins > 65536 || capacity < 0 || ld < shard_geom(n, world, 128).W)
    return fail(DA_ERR_BAD_ARG, "bad shard edge-extraction arguments");
  if (n > 0x7fffffffLL) return fail(DA_ERR_UNSUPPORTED, "edge indices are int32");
  return launch_extract_edges(d_local, ld, n, d_keep, nbins, include_diagonal != 0, d_i, d_j, d_v, capacity,
                              reinterpret_cast<unsigned long long *>(d_count), static_cast<hipStream_t>(stream), rank, world);
}

int da_dev_extract_edges(const uint16_t *d_compact, int64_t ld, int64_t n, const uint8_t *d_keep, int nbins,
                         int include_diagonal, int32_t *d_i, int32_t *d_j, uint16_t *d_v, int64_t capacity,
                         uint64_t *d_count, void *stream) {
  if (n <= 0) return DA_OK;
  if (!d_compact || !d_keep || !d_i || !d_j || !d_v || !d_count || ld < n || nbins <= 0 || nbins > 65536 || capacity < 0)
    return fail(DA_ERR_BAD_ARG, "bad edge-extraction arguments");
  if (n > 0x7fffffffLL) return fail(DA_ERR_UNSUPPORTED, "edge indices are int32");
  return launch_extract_edges(d_compact, ld, n, d_keep, nbins, include_diagonal != 0, d_i, d_j, d_v, capacity,
                              reinterpret_cast<unsigned long long *>(d_count), static_cast<hipStream_t>(stream));
}

// the device edge list (da_dev_extract_edges[_rows]: i <= j, codes) as the symmetric CSR da_louvain_csr clusters -- sorted on the
// device (one radix sort of 2 m keys), so the host neither sorts 1.45e8 edges nor carries 16 bytes per edge
size_t da_dev_edges_to_csr_bytes(int64_t n_edges, int64_t n) { return edges_to_csr_workspace_bytes(n_edges, n); }

int da_dev_edges_to_csr(const int32_t *d_i, const int32_t *d_j, const uint16_t *d_v, int64_t n_edges, int64_t n, void *d_work,
                        size_t work_bytes, int64_t *d_ptr, int32_t *d_adj, uint16_t *d_codes, uint16_t *d_loops, void *stream) {
  if (n <= 0) return fail(DA_ERR_EMPTY_INPUT, "%s", da_status_message(DA_ERR_EMPTY_INPUT));
  if (n_edges < 0 || !d_ptr || !d_loops || (n_edges > 0 && (!d_i || !d_j || !d_v || !d_adj || !d_codes || !d_work)))
    return fail(DA_ERR_BAD_ARG, "bad edges -> CSR arguments");
  if (n_edges > 0 && (reinterpret_cast<uintptr_t>(d_work) & 255)) return fail(DA_ERR_BAD_ARG, "workspace must be 256-byte aligned");
  return launch_edges_to_csr(d_i, d_j, d_v, n_edges, n, d_work, work_bytes, d_ptr, d_adj, d_codes, d_loops, static_cast<hipStream_t>(stream));
}

// ---- the synchronous Louvain (clusterbreak.louvain_sync_dense) on the resident CSR: the graph never crosses to the host ------------------
size_t da_dev_louvain_workspace_bytes(int64_t n, int64_t nnz) { return louvain_device_workspace_bytes(n, nnz); }

int da_dev_louvain_csr(int64_t n, const int64_t *d_ptr, const int32_t *d_adj, const uint16_t *d_codes, const uint16_t *d_loops, const double *values,
                       int32_t n_values, double resolution, uint32_t seed, void *d_work, size_t work_bytes, int32_t *d_membership,
                       double *modularity_out, int32_t *levels_out, int32_t *iterations_out, void *stream) {
  if (n < 0) return fail(DA_ERR_BAD_ARG, "n must not be negative (got %lld)", (long long)n);
  if (levels_out) *levels_out = 0;
  if (modularity_out) *modularity_out = 0.0;
  if (iterations_out) std::fill(iterations_out, iterations_out + 32, 0);
  if (n == 0) return DA_OK;
  if (n > 0x7ffffff0LL) return fail(DA_ERR_UNSUPPORTED, "device Louvain: too many vertices");
  if (!d_ptr || !d_work || !d_membership) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (n_values < 0 || n_values > 65535 || (n_values > 0 && !values))
    return fail(DA_ERR_BAD_ARG, "values must hold 0 .. 65535 weights (got %d)", (int)n_values);
  if (!(resolution >= 0.0) || !std::isfinite(resolution)) return fail(DA_ERR_BAD_ARG, "the resolution must be finite and not negative");
  if (reinterpret_cast<uintptr_t>(d_work) & 255) return fail(DA_ERR_BAD_ARG, "workspace must be 256-byte aligned");
  if (work_bytes < louvain_device_workspace_bytes(n, 0)) return fail(DA_ERR_BAD_ARG, "device Louvain: workspace too small");
  return launch_louvain_device(n, d_ptr, d_adj, d_codes, d_loops, values, n_values, resolution, seed, d_work, work_bytes, d_membership, modularity_out,
                               levels_out, iterations_out, static_cast<hipStream_t>(stream));
}

// ---- connected components (clusterbreak.components_dense) of a resident edge list or CSR: a lock-free union-find, n labels out -----------
size_t da_dev_components_workspace_bytes(int64_t n) { return components_workspace_bytes(n); }

}  // extern "C"  (reopened below)
namespace {
// what the device component calls share: shapes and pointers, before the device is touched.  DA_OK with *done = true: n == 0, nothing to run.
int components_dev_check(int64_t n, const void *d_work, size_t work_bytes, const void *d_membership, int64_t *n_components_out, bool *done) {
  *done = false;
  if (n < 0) return fail(DA_ERR_BAD_ARG, "n must not be negative (got %lld)", (long long)n);
  if (!n_components_out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  *n_components_out = 0;
  if (n == 0) { *done = true; return DA_OK; }
  if (n > 0x7ffffff0LL) return fail(DA_ERR_UNSUPPORTED, "components: too many vertices");
  if (!d_work || !d_membership) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (work_bytes < components_workspace_bytes(n)) return fail(DA_ERR_BAD_ARG, "components: workspace too small");
  return DA_OK;
}
}  // namespace
extern "C" {

int da_dev_components_edges(const int32_t *d_i, const int32_t *d_j, const uint16_t *d_code, int min_code, int64_t n_edges, int64_t n, void *d_work,
                            size_t work_bytes, int32_t *d_membership, int32_t *d_sizes, int64_t *n_components_out, void *stream) {
  int rc;
  bool done;
  if (n_edges < 0) return fail(DA_ERR_BAD_ARG, "negative shape");
  if ((rc = components_dev_check(n, d_work, work_bytes, d_membership, n_components_out, &done)) != DA_OK || done) return rc;
  if (n_edges > 0 && (!d_i || !d_j)) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  return launch_components_edges(d_i, d_j, d_code, min_code, n_edges, n, d_work, work_bytes, d_membership, d_sizes, n_components_out,
                                 static_cast<hipStream_t>(stream));
}

int da_dev_components_csr(int64_t n, const int64_t *d_ptr, const int32_t *d_adj, int symmetric, void *d_work, size_t work_bytes, int32_t *d_membership,
                          int32_t *d_sizes, int64_t *n_components_out, void *stream) {
  int rc;
  bool done;
  if ((rc = components_dev_check(n, d_work, work_bytes, d_membership, n_components_out, &done)) != DA_OK || done) return rc;
  if (!d_ptr) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  return launch_components_csr(n, d_ptr, d_adj, symmetric != 0, d_work, work_bytes, d_membership, d_sizes, n_components_out,
                               static_cast<hipStream_t>(stream));
}

// R's quantile(x, p, type = 7) (stats::quantile.default, the default the reference's
// R/clusterbreak.R:219 uses) of the multiset {values[b] x hist[b]}, values ascending:
//   index = 1 + (N-1) p; lo = floor(index); hi = ceiling(index); q = x[lo];
//   if (index > lo && x[hi] != q) q = (1-h) q + h x[hi],  h = index - lo
int da_quantile_type7(const uint64_t *hist, const double *values, int nbins, double p, double *q_out) {
  if (!hist || !values || !q_out || nbins <= 0 || !(p >= 0.0 && p <= 1.0)) return fail(DA_ERR_BAD_ARG, "bad quantile arguments");
  uint64_t total = 0;
  for (int b = 0; b < nbins; ++b) total += hist[b];
  if (total == 0) return fail(DA_ERR_BAD_ARG, "quantile of an empty set");
  const double index = 1.0 + (double)(total - 1) * p;
  const double lo = std::floor(index), hi = std::ceil(index);
  auto at = [&](double pos1) {  // pos1: 1-based rank
    const uint64_t r = (uint64_t)pos1;
    uint64_t cum = 0;
    for (int b = 0; b < nbins; ++b) {
      cum += hist[b];
      if (r <= cum) return values[b];
    }
    return values[nbins - 1];
  };
  double q = at(lo);
  const double xh = at(hi);
  if (index > lo && xh != q) {
    const double h = index - lo;
    q = (1.0 - h) * q + h * xh;
  }
  *q_out = q;
  return DA_OK;
}

// mean, median, min and max of the multiset {values[b] x hist[b]}, values ascending (dynaalign.h): the numbers of the reference's
// compute_similarity_stats (R/similarity.R:22-25) from a histogram.  The median is R's / numpy's, the plain average of the two middle
// elements; the mean is one long double sum over the bins.
int da_stats_from_histogram(const uint64_t *hist, const double *values, int64_t nbins, double *mean_out, double *median_out, double *min_out,
                            double *max_out) {
  if (!hist || !values || nbins <= 0) return fail(DA_ERR_BAD_ARG, "bad statistics arguments");
  uint64_t total = 0;
  int64_t lo = -1, hi = -1;
  long double sum = 0.0L;
  for (int64_t b = 0; b < nbins; ++b) {
    if (!hist[b]) continue;
    if (lo < 0) lo = b;
    hi = b;
    total += hist[b];
    sum += (long double)hist[b] * (long double)values[b];
  }
  if (total == 0) return fail(DA_ERR_BAD_ARG, "statistics of an empty set");
  auto at = [&](uint64_t pos) {   // pos: 0-based rank
    uint64_t cum = 0;
    for (int64_t b = lo; b <= hi; ++b) {
      cum += hist[b];
      if (pos < cum) return values[b];
    }
    return values[hi];
  };
  if (mean_out) *mean_out = (double)(sum / (long double)total);
  if (median_out) *median_out = (total & 1) ? at((total - 1) / 2) : (at(total / 2 - 1) + at(total / 2)) / 2.0;
  if (min_out) *min_out = values[lo];
  if (max_out) *max_out = values[hi];
  return DA_OK;
}

static int nw_validate(const uint8_t *residues, const int64_t *offsets, int64_t n);

// Shared tail of the *_edges entry points: d_cnt is the dense n x n uint16 code matrix, d_hist the
// histogram of its strict upper triangle (nbins codes), values[b] the similarity a code stands for.
//   threshold <- quantile(S[upper.tri(S)], thresh_p)   (R type 7, R/clusterbreak.R:219)
//   S[S < threshold] <- 0; a zero weight is no edge     (:221; igraph, weighted = TRUE)
// The diagonal (1.0) always survives.  Edges come back sorted by (i, j).
struct EdgeSet {
  double threshold = 0.0;
  std::vector<int32_t> i, j;
  std::vector<double> w;
};

static int edges_from_counts(const uint16_t *d_cnt, int64_t n, int nbins, const unsigned long long *d_hist,
                             const std::vector<double> &values, double thresh_p, bool want_edges, EdgeSet &es,
                             int64_t *n_edges_out) {
  int rc;
  std::vector<uint64_t> h(nbins);
  DA_HIP_TRY(hipMemcpy(h.data(), d_hist, (size_t)nbins * 8, hipMemcpyDeviceToHost));
  // order statistics need the codes in ascending order of their VALUE (MH: already so; NW: ratios)
  std::vector<int> order(nbins);
  for (int b = 0; b < nbins; ++b) order[b] = b;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return values[a] < values[b]; });
  std::vector<uint64_t> hs(nbins);
  std::vector<double> vs(nbins);
  for (int b = 0; b < nbins; ++b) { hs[b] = h[order[b]]; vs[b] = values[order[b]]; }
  double thr;
  if ((rc = da_quantile_type7(hs.data(), vs.data(), nbins, thresh_p, &thr)) != DA_OK) return rc;
  es.threshold = thr;
  std::vector<uint8_t> kp(nbins);
  int64_t n_edges = n;                                                       // the diagonal (1.0) always survives
  for (int b = 0; b < nbins; ++b) {
    kp[b] = (values[b] != 0.0 && !(values[b] < thr)) ? 1 : 0;
    if (kp[b]) n_edges += (int64_t)h[b];
  }
  *n_edges_out = n_edges;
  if (!want_edges || n_edges == 0) return DA_OK;
  DevBuf keep, cnt_edges, di, dj, dv;
  if ((rc = keep.alloc((size_t)nbins)) != DA_OK) return rc;
  if ((rc = cnt_edges.alloc(8)) != DA_OK) return rc;
  if ((rc = di.alloc((size_t)n_edges * 4)) != DA_OK) return rc;
  if ((rc = dj.alloc((size_t)n_edges * 4)) != DA_OK) return rc;
  if ((rc = dv.alloc((size_t)n_edges * 2)) != DA_OK) return rc;
  DA_HIP_TRY(hipMemcpy(keep.p, kp.data(), (size_t)nbins, hipMemcpyHostToDevice));
  DA_HIP_TRY(hipMemset(cnt_edges.p, 0, 8));
  if ((rc = launch_extract_edges(d_cnt, n, n, keep.as<uint8_t>(), nbins, true, di.as<int32_t>(), dj.as<int32_t>(),
                                 dv.as<uint16_t>(), n_edges, cnt_edges.as<unsigned long long>(), nullptr)) != DA_OK) return rc;
  uint64_t got = 0;
  DA_HIP_TRY(hipMemcpy(&got, cnt_edges.p, 8, hipMemcpyDeviceToHost));
  if ((int64_t)got != n_edges) return fail(DA_ERR_HIP, "edge count mismatch: histogram says %lld, extraction found %llu",
                                           (long long)n_edges, (unsigned long long)got);
  std::vector<int32_t> hi_(n_edges), hj_(n_edges);
  std::vector<uint16_t> hv_(n_edges);
  DA_HIP_TRY(hipMemcpy(hi_.data(), di.p, (size_t)n_edges * 4, hipMemcpyDeviceToHost));
  DA_HIP_TRY(hipMemcpy(hj_.data(), dj.p, (size_t)n_edges * 4, hipMemcpyDeviceToHost));
  DA_HIP_TRY(hipMemcpy(hv_.data(), dv.p, (size_t)n_edges * 2, hipMemcpyDeviceToHost));
  // the device appends in arrival order; hand the edges back sorted by (i, j): a counting sort by row (1.45e8 edges at
  // N = 100k: a comparison sort of the whole list took ~20 s on one thread), then every row's columns are sorted -- rows are
  // independent, a few host threads share them; (i, j) pairs are unique, so the order is fully determined
  std::vector<int64_t> rptr((size_t)n + 1, 0);
  for (int64_t e = 0; e < n_edges; ++e) ++rptr[(size_t)hi_[(size_t)e] + 1];
  for (int64_t v = 0; v < n; ++v) rptr[(size_t)v + 1] += rptr[(size_t)v];
  std::vector<int32_t> sj((size_t)n_edges);
  std::vector<uint16_t> sv((size_t)n_edges);
  {
    std::vector<int64_t> cur(rptr.begin(), rptr.end() - 1);
    for (int64_t e = 0; e < n_edges; ++e) {
      const int64_t pos = cur[(size_t)hi_[(size_t)e]]++;
      sj[(size_t)pos] = hj_[(size_t)e];
      sv[(size_t)pos] = hv_[(size_t)e];
    }
  }
  hj_.clear(); hj_.shrink_to_fit(); hv_.clear(); hv_.shrink_to_fit();
  es.i.resize(n_edges); es.j.resize(n_edges); es.w.resize(n_edges);
  {
    unsigned nt = std::thread::hardware_concurrency();
    nt = std::max(1u, std::min(16u, nt ? nt : 1u));
    if (n_edges < 1000000) nt = 1;
    std::vector<std::thread> th;
    auto work = [&](unsigned t) {
      std::vector<std::pair<int32_t, uint16_t>> tmp;
      const int64_t e_lo = n_edges * t / nt, e_hi = n_edges * (t + 1) / nt;      // rows cut at roughly equal edge counts
      int64_t v0 = t == 0 ? 0 : std::lower_bound(rptr.begin(), rptr.end() - 1, e_lo) - rptr.begin();
      int64_t v1 = t + 1 == nt ? n : std::lower_bound(rptr.begin(), rptr.end() - 1, e_hi) - rptr.begin();
      for (int64_t v = v0; v < v1; ++v) {
        const int64_t b = rptr[(size_t)v], e = rptr[(size_t)v + 1];
        tmp.clear();
        for (int64_t q = b; q < e; ++q) tmp.emplace_back(sj[(size_t)q], sv[(size_t)q]);
        std::sort(tmp.begin(), tmp.end());
        for (int64_t q = b; q < e; ++q) {
          es.i[(size_t)q] = (int32_t)v;
          es.j[(size_t)q] = tmp[(size_t)(q - b)].first;
          es.w[(size_t)q] = values[tmp[(size_t)(q - b)].second];
        }
      }
    };
    for (unsigned t = 1; t < nt; ++t) th.emplace_back(work, t);
    work(0);
    for (auto &x : th) x.join();
  }
  return DA_OK;
}

// legacy calling convention of the *_edges entry points on top of an EdgeSet: size query (all buffers NULL) or fill
static int edges_deliver(const EdgeSet &es, int64_t n_edges, double *threshold_out, int64_t *n_edges_out, int64_t capacity,
                         int32_t *ei, int32_t *ej, double *ew) {
  *threshold_out = es.threshold;
  *n_edges_out = n_edges;
  if (!ei && !ej && !ew) return DA_OK;
  if (capacity < n_edges) return fail(DA_ERR_BAD_ARG, "edge buffers hold %lld entries, %lld needed", (long long)capacity, (long long)n_edges);
  if (n_edges) {
    memcpy(ei, es.i.data(), (size_t)n_edges * 4);
    memcpy(ej, es.j.data(), (size_t)n_edges * 4);
    memcpy(ew, es.w.data(), (size_t)n_edges * 8);
  }
  return DA_OK;
}
}  // extern "C"  (reopened below)

struct da_edges { EdgeSet es; int64_t n_edges = 0; };

// ---- what the host-pointer, edge-list and multi-device entry points share
namespace da {
namespace {

int sync_or_fail(const char *what) {
  return hipStreamSynchronize(nullptr) == hipSuccess ? DA_OK : fail(DA_ERR_HIP, "%s", what);
}

// The MinHash preparation on the current device: the uploaded input (in), the signatures (K1) and bit planes (K1b) of up to `cap`
// hash functions at a time, and the planes workspace, held from the first build() (or alloc_work()) to finish().
struct MhPlanes {
  DeviceInput in;
  DevBuf sig, planes, work;
  int64_t n = 0, lds = 0;
  int cap = 0, bits = 32;
  size_t wb = 0;
  int alloc(int64_t n_, int cap_, bool with_planes = true) {
    n = n_; cap = cap_; lds = sig_ld_for(cap);
    int rc = sig.alloc((size_t)n * lds * sizeof(uint32_t));
    if (rc == DA_OK && with_planes) rc = planes.alloc((size_t)mh_planes_words(n, cap) * sizeof(uint32_t));
    return rc;
  }
  int alloc_work() { wb = mh_planes_workspace_bytes(n, cap); return work.alloc(wb); }
  // K1 of hash functions [h0, h0 + nh)
  int signatures(int k, int h0, int nh) {
    return launch_minhash_signatures(in.res.as<uint8_t>(), in.off.as<int64_t>(), n, k, nh, in.seeds.as<uint32_t>() + h0,
                                     sig.as<uint32_t>(), lds, nullptr);
  }
  // K1 + K1b of hash functions [h0, h0 + nh): the planes and their `bits`
  int build(int k, int h0, int nh) {
    int rc;
    if ((rc = signatures(k, h0, nh)) != DA_OK) return rc;
    if (!work.p && (rc = alloc_work()) != DA_OK) return rc;
    return build_planes(sig.as<uint32_t>(), lds, n, nh, 0, work.p, wb, planes.as<uint32_t>(), &bits, nullptr);
  }
  int finish() {
    DA_HIP_TRY(hipStreamSynchronize(nullptr));   // the workspace is released here, before anything measures free memory
    work.release();
    return DA_OK;
  }
};

// The NW preparation on the current device: the uploaded input (in) and its residues encoded for the DP (codes)
struct NwCodes {
  DeviceInput in;
  DevBuf codes, bad;
  int upload(const uint8_t *residues, const int64_t *offsets, int64_t n, int64_t total) {
    int rc;
    if ((rc = in.upload(residues, offsets, n, total, nullptr, 0)) != DA_OK) return rc;
    if ((rc = codes.alloc((size_t)total)) != DA_OK) return rc;
    if ((rc = bad.alloc(sizeof(int32_t))) != DA_OK) return rc;
    DA_HIP_TRY(hipMemsetAsync(bad.p, 0, sizeof(int32_t), nullptr));
    return launch_nw_encode(in.res.as<uint8_t>(), total, codes.as<uint8_t>(), bad.as<int32_t>(), nullptr);
  }
};

// The similarity a uint16 result code stands for.  MinHash: match count c -> c / n_hash (src/minHash.cpp:174).
// NW: (matches << 8 | length) -> matches / length (src/pairwiseSeqAlign.cpp:311), `len0` at length 0.
std::vector<double> mh_code_values(int n_hash) {
  std::vector<double> v((size_t)n_hash + 1);
  for (int c = 0; c <= n_hash; ++c) v[(size_t)c] = (double)c / (double)n_hash;
  return v;
}
std::vector<double> nw_code_values(int count, double len0) {
  std::vector<double> v((size_t)count);
  for (int c = 0; c < count; ++c) {
    const int ln = c & 255;
    v[(size_t)c] = ln ? (double)(c >> 8) / (double)ln : len0;
  }
  return v;
}

// The n x n float64 matrix for a HOST caller as uint16 codes: compute(d) writes them to the device buffer d, a quarter of the bytes
// cross PCIe, and the host widens them while copying, out[i] = table[code[i]] -- the divide behind every table entry is the same IEEE
// operation here as on the device.
template <typename F> int codes_to_host(int64_t n, double *out, const std::vector<double> &table, Trace &tr, F compute) {
  const size_t bytes = (size_t)n * (size_t)n * sizeof(uint16_t);
  DevBuf d;
  int rc;
  if ((rc = d.alloc(bytes)) != DA_OK) return rc;
  if ((rc = compute(d.p)) != DA_OK) return rc;
  if ((rc = d2h_pipelined(out, d.p, bytes, table.data())) != DA_OK) return rc;
  tr.mark("device -> host + widen");
  return DA_OK;
}

// Rows [r0, r1) of a result with `cols` columns (esz bytes per device element) to the host at out, in blocks of as many rows as the device
// holds: compute(b0, b1, d) writes rows [b0, b1) to the device buffer d with leading dimension ld, then they are copied out.  The block
// size is measured here, after the caller's allocations, and depends on the columns only -- a tall result (rows >> cols: the two-set calls)
// is not cut by its column count, and every block starts on a multiple of 128 rows after r0.  compute_ms / d2h_ms, if given, add up the
// time of each step.  table: the device elements are uint16 codes and the host widens them while copying, out (double) = table[code].
// even_ld: ld = cols rounded up to even (what the hand-scheduled compare's stores need), compacted on the device before the copy;
// otherwise ld = cols.
template <typename F> int rows_to_host(int64_t cols, int64_t r0, int64_t r1, size_t esz, void *out, F compute,
                                       double *compute_ms = nullptr, double *d2h_ms = nullptr, const double *table = nullptr,
                                       bool even_ld = false) {
  const int64_t ld = even_ld ? cols + (cols & 1) : cols;
  const bool compact = ld != cols;
  const int64_t blk = std::min(block_rows(compact ? ld + cols : cols, esz), r1 - r0);
  const size_t out_esz = table ? sizeof(double) : esz;
  DevBuf d, dc;
  int rc;
  if ((rc = d.alloc((size_t)blk * (size_t)ld * esz)) != DA_OK) return rc;
  if (compact && (rc = dc.alloc((size_t)blk * (size_t)cols * esz)) != DA_OK) return rc;
  for (int64_t b0 = r0; b0 < r1; b0 += blk) {
    const int64_t b1 = std::min(r1, b0 + blk);
    double t = now_ms();
    if ((rc = compute(b0, b1, d.p)) != DA_OK) return rc;
    if (compact)
      DA_HIP_TRY(hipMemcpy2DAsync(dc.p, (size_t)cols * esz, d.p, (size_t)ld * esz, (size_t)cols * esz, (size_t)(b1 - b0), hipMemcpyDeviceToDevice, nullptr));
    if (compute_ms) *compute_ms += now_ms() - t;
    t = now_ms();
    rc = d2h_pipelined(static_cast<char *>(out) + (size_t)(b0 - r0) * (size_t)cols * out_esz, compact ? dc.p : d.p,
                       (size_t)(b1 - b0) * (size_t)cols * esz, table);
    if (d2h_ms) *d2h_ms += now_ms() - t;
    if (rc != DA_OK) return rc;
  }
  return DA_OK;
}

// The public edge-list forms around core(want_edges, es, &n_edges).  da_similarity_*_edges: size query (buffers NULL) or fill -- each
// call runs the whole pipeline.  da_similarity_*_edges_begin / da_edges_fetch / da_edges_free: ONE pass; the result waits in a handle.
template <typename Core> int edges_run_deliver(double *threshold_out, int64_t *n_edges_out, int64_t capacity, int32_t *ei, int32_t *ej,
                                              double *ew, Core core) {
  if (!threshold_out || !n_edges_out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  if ((ei || ej || ew) && (!ei || !ej || !ew)) return fail(DA_ERR_BAD_ARG, "NULL edge buffer");
  EdgeSet es;
  int64_t m = 0;
  const int rc = core(ei != nullptr, es, &m);
  if (rc != DA_OK) return rc;
  return edges_deliver(es, m, threshold_out, n_edges_out, capacity, ei, ej, ew);
}

template <typename Core> int edges_run_handle(da_edges **handle_out, double *threshold_out, int64_t *n_edges_out, Core core) {
  if (!handle_out || !threshold_out || !n_edges_out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  *handle_out = nullptr;
  std::unique_ptr<da_edges> h(new da_edges);
  const int rc = core(true, h->es, &h->n_edges);
  if (rc != DA_OK) return rc;
  *threshold_out = h->es.threshold;
  *n_edges_out = h->n_edges;
  *handle_out = h.release();
  return DA_OK;
}

}  // namespace
}  // namespace da

extern "C" {

// similarityNW + clusterbreak's threshold step as an edge list.  The uint16 code (matches << 8 | length)
// takes few distinct values, so the same histogram / quantile / extraction path as for MinHash applies;
// value(code) = matches / length with the reference's divide (src/pairwiseSeqAlign.cpp:311).
static int nw_edges_core(const uint8_t *residues, const int64_t *offsets, int64_t n, const char *matrix_name,
                         int gap_open, int gap_ext, double thresh_p, bool want_edges, EdgeSet &es, int64_t *n_edges_out) {
  const int mid = da_matrix_id(matrix_name);  // reference :338 -> :190-206, before anything else
  if (mid < 0) return DA_ERR_BAD_MATRIX;
  if (!residues) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  if (n < 2) return fail(DA_ERR_BAD_ARG, "the threshold is a quantile of the strict upper triangle: need >= 2 sequences");
  if (!(thresh_p >= 0.0 && thresh_p <= 1.0)) return fail(DA_ERR_BAD_ARG, "thresh_p must be in [0, 1]");
  int64_t total, max_len;
  int rc;
  if ((rc = check_offsets(offsets, n, &total, &max_len)) != DA_OK) return rc;
  if ((rc = nw_validate(residues, offsets, n)) != DA_OK) return rc;
  for (int64_t i = 0; i < n; ++i)
    if (offsets[i + 1] == offsets[i])
      return fail(DA_ERR_UNSUPPORTED, "sequence %lld is empty: its similarities are 0/0 = NaN and R's quantile() refuses NaN",
                  (long long)(i + 1));
  if (max_len > 127) return fail(DA_ERR_UNSUPPORTED, "the NW edge list works on uint16 codes: sequences up to 127 residues");
  if ((rc = require_device()) != DA_OK) return rc;
  NwCodes nw;
  DevBuf cnt, hist;
  if ((rc = nw.upload(residues, offsets, n, total)) != DA_OK) return rc;
  if ((rc = cnt.alloc((size_t)n * (size_t)n * 2)) != DA_OK) return rc;      // uint16 codes stay on the device
  const int nbins = (int)((max_len << 8) | (2 * max_len)) + 1;              // matches <= max_len, length <= 2 * max_len
  if ((rc = hist.alloc((size_t)nbins * 8)) != DA_OK) return rc;
  DA_HIP_TRY(hipMemset(hist.p, 0, (size_t)nbins * 8));
  if ((rc = nw_full_symmetric(nw.codes.as<uint8_t>(), nw.in.off.as<int64_t>(), n, total, max_len, mid, gap_open, gap_ext, DA_OUT_COMPACT,
                              cnt.p, n, nullptr)) != DA_OK) return rc;
  if ((rc = launch_upper_histogram(cnt.as<uint16_t>(), n, n, nbins, hist.as<unsigned long long>(), nullptr)) != DA_OK) return rc;
  // length 0 cannot occur (no empty sequences)
  return edges_from_counts(cnt.as<uint16_t>(), n, nbins, hist.as<unsigned long long>(), nw_code_values(nbins, 0.0), thresh_p, want_edges,
                           es, n_edges_out);
}

static int mh_edges_core(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, int n_hash,
                         const uint32_t *seeds, double thresh_p, bool want_edges, EdgeSet &es, int64_t *n_edges_out) {
  int rc = validate_mh(n, k, n_hash);
  if (rc != DA_OK) return rc;
  if (!residues || !seeds) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  if (n < 2) return fail(DA_ERR_BAD_ARG, "the threshold is a quantile of the strict upper triangle: need >= 2 sequences");
  if (!(thresh_p >= 0.0 && thresh_p <= 1.0)) return fail(DA_ERR_BAD_ARG, "thresh_p must be in [0, 1]");
  if (n_hash > 65535) return fail(DA_ERR_UNSUPPORTED, "the compare kernel counts in 16 bits: n_hash <= 65535 (got %d)", n_hash);
  int64_t total, max_len;
  if ((rc = check_offsets(offsets, n, &total, &max_len)) != DA_OK) return rc;
  if ((rc = require_device()) != DA_OK) return rc;
  MhPlanes mh;
  DevBuf cnt, hist;
  if ((rc = mh.in.upload(residues, offsets, n, total, seeds, n_hash)) != DA_OK) return rc;
  if ((rc = mh.alloc(n, n_hash)) != DA_OK) return rc;
  if ((rc = cnt.alloc((size_t)n * (size_t)n * 2)) != DA_OK) return rc;   // uint16 counts stay on the device
  const int nbins = n_hash + 1;
  if ((rc = hist.alloc((size_t)nbins * 8)) != DA_OK) return rc;
  DA_HIP_TRY(hipMemset(hist.p, 0, (size_t)nbins * 8));
  if ((rc = mh.build(k, 0, n_hash)) != DA_OK || (rc = mh.finish()) != DA_OK) return rc;
  if ((rc = launch_mh_compare(mh.planes.as<uint32_t>(), n, n_hash, 0, n, true, DA_OUT_COMPACT, cnt.p, n, nullptr, mh.bits)) != DA_OK)
    return rc;
  if ((rc = launch_upper_histogram(cnt.as<uint16_t>(), n, n, nbins, hist.as<unsigned long long>(), nullptr)) != DA_OK) return rc;
  return edges_from_counts(cnt.as<uint16_t>(), n, nbins, hist.as<unsigned long long>(), mh_code_values(n_hash), thresh_p, want_edges, es,
                           n_edges_out);
}

int da_similarity_nw_edges(const uint8_t *residues, const int64_t *offsets, int64_t n, const char *matrix_name,
                           int gap_open, int gap_ext, double thresh_p, double *threshold_out, int64_t *n_edges_out,
                           int64_t capacity, int32_t *ei, int32_t *ej, double *ew) {
  return edges_run_deliver(threshold_out, n_edges_out, capacity, ei, ej, ew, [&](bool want_edges, EdgeSet &es, int64_t *m) {
    return nw_edges_core(residues, offsets, n, matrix_name, gap_open, gap_ext, thresh_p, want_edges, es, m);
  });
}

int da_similarity_mh_edges(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, int n_hash,
                           const uint32_t *seeds, double thresh_p, double *threshold_out, int64_t *n_edges_out,
                           int64_t capacity, int32_t *ei, int32_t *ej, double *ew) {
  return edges_run_deliver(threshold_out, n_edges_out, capacity, ei, ej, ew, [&](bool want_edges, EdgeSet &es, int64_t *m) {
    return mh_edges_core(residues, offsets, n, k, n_hash, seeds, thresh_p, want_edges, es, m);
  });
}

int da_similarity_mh_edges_begin(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, int n_hash,
                                 const uint32_t *seeds, double thresh_p, da_edges **handle_out, double *threshold_out,
                                 int64_t *n_edges_out) {
  return edges_run_handle(handle_out, threshold_out, n_edges_out, [&](bool want_edges, EdgeSet &es, int64_t *m) {
    return mh_edges_core(residues, offsets, n, k, n_hash, seeds, thresh_p, want_edges, es, m);
  });
}

int da_similarity_nw_edges_begin(const uint8_t *residues, const int64_t *offsets, int64_t n, const char *matrix_name,
                                 int gap_open, int gap_ext, double thresh_p, da_edges **handle_out, double *threshold_out,
                                 int64_t *n_edges_out) {
  return edges_run_handle(handle_out, threshold_out, n_edges_out, [&](bool want_edges, EdgeSet &es, int64_t *m) {
    return nw_edges_core(residues, offsets, n, matrix_name, gap_open, gap_ext, thresh_p, want_edges, es, m);
  });
}

int da_edges_fetch(const da_edges *h, int64_t capacity, int32_t *ei, int32_t *ej, double *ew) {
  if (!h || !ei || !ej || !ew) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  double thr;
  int64_t m;
  return edges_deliver(h->es, h->n_edges, &thr, &m, capacity, ei, ej, ew);
}

void da_edges_free(da_edges *h) { delete h; }


int64_t da_sig_ld(int n_hash) { return sig_ld_for(n_hash); }

// -------------------------------------------------------------- host entry

int da_minhash_signatures(const uint8_t *residues, const int64_t *offsets, int64_t n, int k,
                          int n_hash, const uint32_t *seeds, uint32_t *sig_out) {
  int rc = validate_mh(n, k, n_hash);
  if (rc != DA_OK) return rc;
  if (!residues || !seeds || !sig_out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  int64_t total, max_len;
  if ((rc = check_offsets(offsets, n, &total, &max_len)) != DA_OK) return rc;
  if ((rc = require_device()) != DA_OK) return rc;
  MhPlanes mh;
  if ((rc = mh.in.upload(residues, offsets, n, total, seeds, n_hash)) != DA_OK) return rc;
  if ((rc = mh.alloc(n, n_hash, false)) != DA_OK || (rc = mh.signatures(k, 0, n_hash)) != DA_OK) return rc;
  DA_HIP_TRY(hipMemcpy2D(sig_out, (size_t)n_hash * 4, mh.sig.p, (size_t)mh.lds * 4, (size_t)n_hash * 4, (size_t)n,
                         hipMemcpyDeviceToHost));
  return DA_OK;
}

// similarityMH with more hash functions than the compare kernels' 16-bit counters hold (n_hash > 65535; the reference has
// no limit, src/minHash.cpp:129-131 only asks for > 0): chunks of <= 65504 hash functions go through K1 / K1b / K2 (uint16
// counts) one after the other, the counts are summed in 32 bits on the device and divided by n_hash once.  Needs the whole
// n x n count matrix resident (4 + 2 + 8 bytes per pair).
static int mh_host_chunked(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, int n_hash, const uint32_t *seeds,
                           double *out) {
  constexpr int CHUNK = 65504;                              // a multiple of 32 below 65536
  int64_t total, max_len;
  int rc;
  if ((rc = check_offsets(offsets, n, &total, &max_len)) != DA_OK) return rc;
  if ((rc = require_device()) != DA_OK) return rc;
  if (rows_per_block(n, 4 + 2 + 8) < n)
    return fail(DA_ERR_UNSUPPORTED, "n_hash = %d (> 65535) needs the %lld x %lld count matrix resident in HBM (14 bytes per pair)", n_hash,
                (long long)n, (long long)n);
  MhPlanes mh;
  DevBuf acc, cnt, dout;
  if ((rc = mh.in.upload(residues, offsets, n, total, seeds, n_hash)) != DA_OK) return rc;
  if ((rc = mh.alloc(n, CHUNK)) != DA_OK || (rc = mh.alloc_work()) != DA_OK) return rc;
  if ((rc = acc.alloc((size_t)n * (size_t)n * 4)) != DA_OK) return rc;
  if ((rc = cnt.alloc((size_t)n * (size_t)n * 2)) != DA_OK) return rc;
  for (int h0 = 0; h0 < n_hash; h0 += CHUNK) {
    const int nh = std::min(CHUNK, n_hash - h0);
    if ((rc = mh.build(k, h0, nh)) != DA_OK) return rc;
    if ((rc = launch_mh_compare(mh.planes.as<uint32_t>(), n, nh, 0, n, true, DA_OUT_COMPACT, cnt.p, n, nullptr, mh.bits)) != DA_OK) return rc;
    if ((rc = launch_acc_counts(acc.as<uint32_t>(), cnt.as<uint16_t>(), n * n, h0 == 0, nullptr)) != DA_OK) return rc;
  }
  if ((rc = dout.alloc((size_t)n * (size_t)n * 8)) != DA_OK) return rc;
  if ((rc = launch_counts32_to_f64(acc.as<uint32_t>(), dout.as<double>(), n * n, n_hash, nullptr)) != DA_OK) return rc;
  rc = d2h_pipelined(out, dout.p, (size_t)n * (size_t)n * 8);
  DA_HIP_TRY(hipDeviceSynchronize());
  return rc;
}

static int mh_host_common(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, int n_hash,
                          const uint32_t *seeds, int64_t row_begin, int64_t row_end, int kind, void *out) {
  int rc = validate_mh(n, k, n_hash);
  if (rc != DA_OK) return rc;
  if (!residues || !seeds || !out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  if (row_begin < 0 || row_end > n || row_begin > row_end) return fail(DA_ERR_BAD_ARG, "bad row range");
  if (n_hash > 65535 && kind == DA_OUT_F64 && row_begin == 0 && row_end == n)
    return mh_host_chunked(residues, offsets, n, k, n_hash, seeds, static_cast<double *>(out));
  if (n_hash > 65535)
    return fail(DA_ERR_UNSUPPORTED, "uint16 match counts cannot hold n_hash = %d (> 65535); da_similarity_mh handles it", n_hash);
  int64_t total, max_len;
  if ((rc = check_offsets(offsets, n, &total, &max_len)) != DA_OK) return rc;
  if ((rc = require_device()) != DA_OK) return rc;
  Trace tr("similarityMH host path");
  MhPlanes mh;
  if ((rc = mh.in.upload(residues, offsets, n, total, seeds, n_hash)) != DA_OK) return rc;
  if ((rc = mh.alloc(n, n_hash)) != DA_OK) return rc;
  tr.mark("upload + small allocations");
  if ((rc = mh.build(k, 0, n_hash)) != DA_OK || (rc = mh.finish()) != DA_OK) return rc;
  tr.mark("signatures + codes");
  if (kind == DA_OUT_F64 && row_begin == 0 && row_end == n && rows_per_block(n, sizeof(uint16_t)) >= n && !da::config().no_host_widen)
    return codes_to_host(n, static_cast<double *>(out), mh_code_values(n_hash), tr, [&](void *d) {
      const int rc = launch_mh_compare(mh.planes.as<uint32_t>(), n, n_hash, 0, n, true, DA_OUT_COMPACT, d, n, nullptr, mh.bits);
      if (rc == DA_OK) tr.mark("compare (uint16 counts)");
      return rc;
    });
  const size_t esz = kind == DA_OUT_F64 ? sizeof(double) : sizeof(uint16_t);
  bool whole = false;   // everything fits: compare only the upper triangle, store both halves
  rc = rows_to_host(n, row_begin, row_end, esz, out, [&](int64_t b0, int64_t b1, void *d) {
    whole = b0 == 0 && b1 == n;
    if (b0 == row_begin) tr.mark(whole ? "result allocation (whole)" : "result allocation (row blocks)");
    const int rc = launch_mh_compare(mh.planes.as<uint32_t>(), n, n_hash, b0, b1, whole, kind, d, n, nullptr, mh.bits);
    if (rc == DA_OK && whole) tr.mark("compare");
    return rc;
  });
  if (rc == DA_OK && whole) tr.mark("device -> host");
  return rc;
}

int da_similarity_mh(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, int n_hash,
                     const uint32_t *seeds, double *out) {
  return mh_host_common(residues, offsets, n, k, n_hash, seeds, 0, n > 0 ? n : 0, DA_OUT_F64, out);
}

int da_mh_counts(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, int n_hash,
                 const uint32_t *seeds, int64_t row_begin, int64_t row_end, uint16_t *counts_out) {
  return mh_host_common(residues, offsets, n, k, n_hash, seeds, row_begin, row_end, DA_OUT_COMPACT, counts_out);
}

// Residue validation with the reference's laziness (src/pairwiseSeqAlign.cpp:238-250):
// pairs are visited i ascending, j from i; inside a pair, sequence1[r] is checked at
// the start of DP row r+1, and all of sequence2 is scanned during DP row 1.  A pair
// with an empty sequence1 checks nothing.  Hence the first error raised is for the
// pair (i0, jb): i0 = first non-empty sequence, jb = first sequence holding an
// invalid byte (jb >= i0 necessarily).
static int nw_validate(const uint8_t *residues, const int64_t *offsets, int64_t n) {
  static const char order[] = "ARNDCQEGHILKMFPSTWYVBZX*";
  auto valid = [&](uint8_t c) { return c != 0 && strchr(order, c) != nullptr; };
  int64_t i0 = -1, jb = -1;
  for (int64_t i = 0; i < n && (i0 < 0 || jb < 0); ++i) {
    const int64_t b = offsets[i], e = offsets[i + 1];
    if (i0 < 0 && e > b) i0 = i;
    if (jb < 0)
      for (int64_t p = b; p < e; ++p)
        if (!valid(residues[p])) { jb = i; break; }
  }
  if (jb < 0) return DA_OK;
  const uint8_t *s2 = residues + offsets[jb];
  const int64_t n2 = offsets[jb + 1] - offsets[jb];
  if (jb == i0 && !valid(s2[0]))
    return fail(DA_ERR_BAD_RESIDUE_SEQ1, "Invalid amino acid in sequence1: %c", (char)s2[0]);
  for (int64_t p = 0; p < n2; ++p)
    if (!valid(s2[p])) return fail(DA_ERR_BAD_RESIDUE_SEQ2, "Invalid amino acid in sequence2: %c", (char)s2[p]);
  return DA_OK;  // unreachable
}

static int nw_host_common(const uint8_t *residues, const int64_t *offsets, int64_t n,
                          const char *matrix_name, int gap_open, int gap_ext, int64_t row_begin,
                          int64_t row_end, double *out_f64, int32_t *matches_out, int32_t *len_out,
                          int32_t *score_out) {
  const int mid = da_matrix_id(matrix_name);  // reference :338 -> :190-206, before anything else
  if (mid < 0) return DA_ERR_BAD_MATRIX;
  if (n <= 0) return DA_OK;                    // reference returns a 0x0 matrix
  if (!residues) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  if (row_begin < 0 || row_end > n || row_begin > row_end) return fail(DA_ERR_BAD_ARG, "bad row range");
  int64_t total, max_len;
  int rc;
  if ((rc = check_offsets(offsets, n, &total, &max_len)) != DA_OK) return rc;
  if ((rc = nw_validate(residues, offsets, n)) != DA_OK) return rc;
  if ((rc = require_device()) != DA_OK) return rc;
  Trace tr("similarityNW host path");
  NwCodes nw;
  if ((rc = nw.upload(residues, offsets, n, total)) != DA_OK) return rc;
  const uint8_t *codes = nw.codes.as<uint8_t>();
  const int64_t *d_off = nw.in.off.as<int64_t>();

  if (out_f64 && row_begin == 0 && row_end == n && max_len <= 127 && rows_per_block(n, sizeof(uint16_t)) >= n &&
      !da::config().no_host_widen) {
    const uint64_t nan_bits = 0xFFF8000000000000ULL;        // 0/0 as the reference's x86 host produces it
    double nan;
    memcpy(&nan, &nan_bits, 8);
    return codes_to_host(n, out_f64, nw_code_values(65536, nan), tr, [&](void *d) -> int {
      tr.mark("validation + upload + allocations");
      const int rc = nw_full_symmetric(codes, d_off, n, total, max_len, mid, gap_open, gap_ext, DA_OUT_COMPACT, d, n, nullptr);
      if (rc != DA_OK) return rc;
      if (tr.on) {
        const NwRoute &r = nw_route();
        fprintf(stderr, "[dynaalign]   (plan %.2f ms, DP %.2f ms, expansion %.2f ms; %lld unique of %lld)\n", r.plan_ms, r.dp_ms, r.expand_ms,
                (long long)r.unique, (long long)r.n);
      }
      tr.mark("codes on the device (uint16)");
      return DA_OK;
    });
  }
  if (out_f64)
    return rows_to_host(n, row_begin, row_end, sizeof(double), out_f64, [&](int64_t b0, int64_t b1, void *d) {
      if (b0 == 0 && b1 == n)   // everything fits
        return nw_full_symmetric(codes, d_off, n, total, max_len, mid, gap_open, gap_ext, DA_OUT_F64, d, n, nullptr);
      return launch_nw(codes, d_off, n, max_len, mid, gap_open, gap_ext, b0, b1, false, DA_OUT_F64, d, n, nullptr, 0, nullptr);
    });
  // integer outputs: 32-bit packed (matches<<16|len) + score, unpacked on the host
  const int64_t rows_total = row_end - row_begin;
  const int64_t blk = rows_per_block(n, sizeof(uint32_t) + sizeof(int32_t));
  DevBuf dpk, dsc;
  const int64_t brow = std::min(blk, rows_total);
  if ((rc = dpk.alloc((size_t)brow * (size_t)n * sizeof(uint32_t))) != DA_OK) return rc;
  if (score_out && (rc = dsc.alloc((size_t)brow * (size_t)n * sizeof(int32_t))) != DA_OK) return rc;
  std::vector<uint32_t> hpk((size_t)brow * (size_t)n);
  for (int64_t r0 = row_begin; r0 < row_end; r0 += blk) {
    const int64_t r1 = std::min(row_end, r0 + blk);
    const bool whole = (r0 == 0 && r1 == n);
    rc = launch_nw(codes, d_off, n, max_len, mid, gap_open, gap_ext, r0, r1, whole,
                   DA_OUT_PACK32, dpk.p, n, score_out ? dsc.as<int32_t>() : nullptr, n, nullptr);
    if (rc != DA_OK) return rc;
    const size_t cnt = (size_t)(r1 - r0) * (size_t)n, base = (size_t)(r0 - row_begin) * (size_t)n;
    DA_HIP_TRY(hipMemcpy(hpk.data(), dpk.p, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t e = 0; e < cnt; ++e) {
      if (matches_out) matches_out[base + e] = (int32_t)(hpk[e] >> 16);
      if (len_out) len_out[base + e] = (int32_t)(hpk[e] & 0xffffu);
    }
    if (score_out) DA_HIP_TRY(hipMemcpy(score_out + base, dsc.p, cnt * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  return DA_OK;
}

int da_similarity_nw(const uint8_t *residues, const int64_t *offsets, int64_t n, const char *matrix_name,
                     int gap_open, int gap_ext, double *out) {
  if (n > 0 && !out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  return nw_host_common(residues, offsets, n, matrix_name, gap_open, gap_ext, 0, n > 0 ? n : 0, out, nullptr,
                        nullptr, nullptr);
}

int da_nw_pairs(const uint8_t *residues, const int64_t *offsets, int64_t n, const char *matrix_name,
                int gap_open, int gap_ext, int64_t row_begin, int64_t row_end, int32_t *matches_out,
                int32_t *len_out, int32_t *score_out) {
  return nw_host_common(residues, offsets, n, matrix_name, gap_open, gap_ext, row_begin, row_end, nullptr,
                        matches_out, len_out, score_out);
}

// ---- two sets on the host boundary: x (m sequences) against y (n sequences) ------------------------------------------------------------------
// what both two-set MinHash host calls check before a device is needed: x empty, y empty, k, n_hash, pointers, the 16-bit limit, the offsets
static int mh_cross_host_validate(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues, const int64_t *y_offsets,
                                  int64_t n, int k, int n_hash, const uint32_t *seeds, const void *out, int64_t *x_total, int64_t *y_total) {
  int rc;
  if ((rc = validate_mh(m, k > 0 ? k : 1, n_hash > 0 ? n_hash : 1)) != DA_OK || (rc = validate_mh(n, k, n_hash)) != DA_OK) return rc;   // x empty, y empty, k, n_hash
  if (!x_residues || !y_residues || !seeds || !out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  if (n_hash > 65535) return fail(DA_ERR_UNSUPPORTED, "the two-set calls take n_hash <= 65535 (got %d)", n_hash);
  int64_t max_len;
  if ((rc = check_offsets(x_offsets, m, x_total, &max_len)) != DA_OK || (rc = check_offsets(y_offsets, n, y_total, &max_len)) != DA_OK) return rc;
  return DA_OK;
}
// similarityMH for two sets: out[i][j] = #{h : sig_x[i][h] == sig_y[j][h]} / n_hash, no forced diagonal.  column_major: out[i + j * m]
// (R's NumericMatrix(m, n)) -- the similarity is symmetric, so that is the row-major result of y against x.
int da_similarity_mh_cross(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues, const int64_t *y_offsets,
                           int64_t n, int k, int n_hash, const uint32_t *seeds, double *out, int column_major) {
  int rc;
  int64_t x_total, y_total;
  if ((rc = mh_cross_host_validate(x_residues, x_offsets, m, y_residues, y_offsets, n, k, n_hash, seeds, out, &x_total, &y_total)) != DA_OK) return rc;
  if ((rc = require_device()) != DA_OK) return rc;
  DeviceInput dx, dy;
  if ((rc = dx.upload(x_residues, x_offsets, m, x_total, seeds, n_hash)) != DA_OK || (rc = dy.upload(y_residues, y_offsets, n, y_total, nullptr, 0)) != DA_OK)
    return rc;
  const DeviceInput &rowset = column_major ? dy : dx, &colset = column_major ? dx : dy;
  const int64_t rows = column_major ? n : m, cols = column_major ? m : n;
  MhCrossOperand c;
  if ((rc = mh_cross_operand(rowset.res.as<uint8_t>(), rowset.off.as<int64_t>(), rows, colset.res.as<uint8_t>(), colset.off.as<int64_t>(), cols, k,
                             n_hash, dx.seeds.as<uint32_t>(), &c, nullptr)) != DA_OK) return rc;
  DA_HIP_TRY(hipStreamSynchronize(nullptr));
  c.work.release(); c.sig.release();                     // before the result blocks are sized
  const std::vector<double> table = mh_code_values(n_hash);
  const bool widen = !da::config().no_host_widen;
  return rows_to_host(cols, 0, rows, widen ? sizeof(uint16_t) : sizeof(double), out, [&](int64_t b0, int64_t b1, void *d) {
    return mh_cross_compare(c, n_hash, b0, b1, widen ? DA_OUT_COMPACT : DA_OUT_F64, d, cols + (cols & 1), nullptr);
  }, nullptr, nullptr, widen ? table.data() : nullptr, true);
}

// What the reference's lazy fill would raise first with the pairs visited i ascending over x, j ascending over y (src/pairwiseSeqAlign.cpp:
// 238-250 per pair: sequence1[0], every character of sequence2, then sequence1[1], ...; an empty sequence1 runs no row and checks nothing, an
// empty sequence2 still has all of sequence1 checked).  Everything hinges on the first non-empty x[i0]: its pairs scan every y[j], and after its
// row only characters of later x[i] can be wrong.
static int nw_cross_validate(const uint8_t *xr, const int64_t *xo, int64_t m, const uint8_t *yr, const int64_t *yo, int64_t n) {
  static const char order[] = "ARNDCQEGHILKMFPSTWYVBZX*";
  auto valid = [&](uint8_t ch) { return ch != 0 && strchr(order, ch) != nullptr; };
  auto seq1 = [&](uint8_t ch) { return fail(DA_ERR_BAD_RESIDUE_SEQ1, "Invalid amino acid in sequence1: %c", (char)ch); };
  auto seq2 = [&](uint8_t ch) { return fail(DA_ERR_BAD_RESIDUE_SEQ2, "Invalid amino acid in sequence2: %c", (char)ch); };
  int64_t i0 = 0;
  while (i0 < m && xo[i0 + 1] == xo[i0]) ++i0;
  if (i0 == m || n <= 0) return DA_OK;
  const uint8_t *s1 = xr + xo[i0];
  const int64_t l1 = xo[i0 + 1] - xo[i0];
  if (!valid(s1[0])) return seq1(s1[0]);                                                   // pair (i0, 0), row 1
  for (int64_t p = yo[0]; p < yo[1]; ++p) if (!valid(yr[p])) return seq2(yr[p]);           // ... its scan of y[0]
  for (int64_t r = 1; r < l1; ++r) if (!valid(s1[r])) return seq1(s1[r]);                  // ... its later rows
  for (int64_t p = yo[1]; p < yo[n]; ++p) if (!valid(yr[p])) return seq2(yr[p]);           // pairs (i0, 1 ..)
  for (int64_t p = xo[i0 + 1]; p < xo[m]; ++p) if (!valid(xr[p])) return seq1(xr[p]);      // rows after i0: y is clean
  return DA_OK;
}

// What the NW two-set host calls share once their own empty shapes are dealt with, in the documented order.  check(): NULL pointers, the
// offsets, the residues (nw_cross_validate), the caller's own argument checks (`extra`), then -- for the calls that order the values
// (nan_tail: "an order", "a quantile"; NULL: empty sequences are accepted) -- no empty sequence, and the longest sequence against len_limit
// (0: none) with the caller's limit_text.  upload(): DA_ERR_NO_DEVICE last, then the two sets as ONE encoded code buffer [x ; y] on the device
// (m + n sequences), of which the device evaluates pair (p, q) as calc(seq[min(p, q)], seq[max(p, q)]): sequence1 is the x string either way.
struct NwCross {
  const uint8_t *xr, *yr;
  const int64_t *xo, *yo;
  int64_t m, n;
  int mid, gap_open, gap_ext;
  int64_t x_total = 0, y_total = 0, max_len = 0;
  NwCodes nw;
  int check(bool out_ok, const std::function<int()> &extra, const char *nan_tail, int64_t len_limit, const char *limit_text) {
    if (!xr || !yr || !out_ok) return fail(DA_ERR_BAD_ARG, "NULL pointer");
    int64_t x_max, y_max;
    int rc;
    if ((rc = check_offsets(xo, m, &x_total, &x_max)) != DA_OK || (rc = check_offsets(yo, n, &y_total, &y_max)) != DA_OK) return rc;
    if ((rc = nw_cross_validate(xr, xo, m, yr, yo, n)) != DA_OK) return rc;
    if (extra && (rc = extra()) != DA_OK) return rc;
    for (int64_t i = 0; nan_tail && i < m + n; ++i) {
      const int64_t *o = i < m ? xo + i : yo + (i - m);
      if (o[1] == o[0])
        return fail(DA_ERR_UNSUPPORTED, "sequence %lld of %s is empty: its similarities are NaN / 0.0 and a NaN has no place in %s",
                    (long long)((i < m ? i : i - m) + 1), i < m ? "x" : "y", nan_tail);
    }
    max_len = std::max(x_max, y_max);
    if (len_limit && max_len > len_limit) return fail(DA_ERR_UNSUPPORTED, "%s", limit_text);
    return DA_OK;
  }
  int upload() {
    int rc;
    if ((rc = require_device()) != DA_OK) return rc;
    std::vector<uint8_t> res((size_t)(x_total + y_total) + 1);
    std::vector<int64_t> off((size_t)(m + n) + 1);
    if (x_total) memcpy(res.data(), xr, (size_t)x_total);
    if (y_total) memcpy(res.data() + x_total, yr, (size_t)y_total);
    for (int64_t i = 0; i <= m; ++i) off[(size_t)i] = xo[i];
    for (int64_t j = 1; j <= n; ++j) off[(size_t)(m + j)] = x_total + yo[j];
    return nw.upload(res.data(), off.data(), m + n, x_total + y_total);
  }
  // rows [b0, b1) of x against the columns of y (the row-major m x n result) ...
  int rows(int64_t b0, int64_t b1, int kind, void *d, int64_t ld, hipStream_t stream) const {
    return launch_nw_rect(nw.codes.as<uint8_t>(), nw.in.off.as<int64_t>(), m + n, max_len, mid, gap_open, gap_ext, b0, b1, m, m + n, kind, d, ld, stream);
  }
  // ... and rows [b0, b1) of y against the columns of x: its transpose, R's column-major NumericMatrix(m, n)
  int rows_of_y(int64_t b0, int64_t b1, int kind, void *d, int64_t ld, hipStream_t stream) const {
    return launch_nw_rect(nw.codes.as<uint8_t>(), nw.in.off.as<int64_t>(), m + n, max_len, mid, gap_open, gap_ext, m + b0, m + b1, 0, m, kind, d, ld, stream);
  }
};

// similarityNW for two sets: out[i][j] = calc(x[i], y[j]) with x[i] as sequence1.  Both sets are encoded into ONE code buffer [x ; y]; the
// device evaluates pair (p, q) of it as calc(seq[min(p, q)], seq[max(p, q)]), so rows of x against columns of y give the row-major result and
// rows of y against columns of x the column-major one (R's NumericMatrix(m, n)) -- sequence1 is the x string either way.
int da_similarity_nw_cross(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues, const int64_t *y_offsets,
                           int64_t n, const char *matrix_name, int gap_open, int gap_ext, double *out, int column_major) {
  const int mid = da_matrix_id(matrix_name);             // before anything else, as in similarityNW
  if (mid < 0) return DA_ERR_BAD_MATRIX;
  if (m <= 0 || n <= 0) return DA_OK;                    // an m x 0 or 0 x n matrix: nothing to write
  NwCross c{x_residues, y_residues, x_offsets, y_offsets, m, n, mid, gap_open, gap_ext};
  int rc;
  if ((rc = c.check(out != nullptr, nullptr, nullptr, 0, nullptr)) != DA_OK || (rc = c.upload()) != DA_OK) return rc;
  const int64_t rows = column_major ? n : m, cols = column_major ? m : n;
  const bool compact = c.max_len <= 127 && !da::config().no_host_widen;
  const uint64_t nan_bits = 0xFFF8000000000000ULL;        // 0/0 as the reference's x86 host produces it
  double nan;
  memcpy(&nan, &nan_bits, 8);
  const std::vector<double> table = compact ? nw_code_values(65536, nan) : std::vector<double>();
  return rows_to_host(cols, 0, rows, compact ? sizeof(uint16_t) : sizeof(double), out, [&](int64_t b0, int64_t b1, void *d) {
    const int kind = compact ? DA_OUT_COMPACT : DA_OUT_F64;
    return column_major ? c.rows_of_y(b0, b1, kind, d, cols, nullptr) : c.rows(b0, b1, kind, d, cols, nullptr);
  }, nullptr, nullptr, compact ? table.data() : nullptr);
}


// ---- two sets, top-k per row on the host boundary (the device part: topk_blocks) -------------------------------------------------------------
// the selection's results to the host: idx as it is, val_out[i][t] = table[key[i][t]] -- the same table the dense calls widen with
static int topk_to_host(const DevBuf &didx, const DevBuf &dkey, int64_t m, int top, const std::vector<double> &table, int32_t *idx_out,
                        double *val_out) {
  const size_t cnt = (size_t)m * (size_t)top;
  DA_HIP_TRY(hipMemcpy(idx_out, didx.p, cnt * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (!val_out) return DA_OK;
  std::vector<uint16_t> key(cnt);
  DA_HIP_TRY(hipMemcpy(key.data(), dkey.p, cnt * sizeof(uint16_t), hipMemcpyDeviceToHost));
  for (size_t e = 0; e < cnt; ++e) val_out[e] = table[key[e]];
  return DA_OK;
}

int da_similarity_mh_cross_topk(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues, const int64_t *y_offsets,
                                int64_t n, int k, int n_hash, const uint32_t *seeds, int top, int32_t *idx_out, double *val_out) {
  int rc;
  int64_t x_total, y_total;
  if ((rc = mh_cross_host_validate(x_residues, x_offsets, m, y_residues, y_offsets, n, k, n_hash, seeds, idx_out, &x_total, &y_total)) != DA_OK) return rc;
  if ((rc = topk_check(top, n)) != DA_OK) return rc;
  if ((rc = require_device()) != DA_OK) return rc;
  DeviceInput dx, dy;
  if ((rc = dx.upload(x_residues, x_offsets, m, x_total, seeds, n_hash)) != DA_OK || (rc = dy.upload(y_residues, y_offsets, n, y_total, nullptr, 0)) != DA_OK)
    return rc;
  MhCrossOperand c;
  DevBuf didx, dkey;
  if ((rc = mh_cross_operand(dx.res.as<uint8_t>(), dx.off.as<int64_t>(), m, dy.res.as<uint8_t>(), dy.off.as<int64_t>(), n, k, n_hash,
                             dx.seeds.as<uint32_t>(), &c, nullptr)) != DA_OK) return rc;
  if ((rc = didx.alloc((size_t)m * (size_t)top * sizeof(int32_t))) != DA_OK || (rc = dkey.alloc((size_t)m * (size_t)top * sizeof(uint16_t))) != DA_OK) return rc;
  if ((rc = mh_cross_topk(c, n_hash, top, didx.as<int32_t>(), top, dkey.as<uint16_t>(), top, nullptr)) != DA_OK) return rc;
  return topk_to_host(didx, dkey, m, top, mh_code_values(n_hash), idx_out, val_out);
}

// rank_out[code] = dense rank of the double value of an NW code among the codes sequences up to max_len residues can produce (dynaalign.h)
int da_nw_code_ranks(int max_len, uint16_t *rank_out, int *distinct_out) {
  if (!rank_out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  if (max_len < 1 || max_len > 127) return fail(DA_ERR_BAD_ARG, "max_len must be in 1 .. 127 (got %d)", max_len);
  std::vector<std::pair<double, int>> v;
  for (int ln = 1; ln <= 2 * max_len; ++ln)
    for (int mt = 0; mt <= std::min(ln, max_len); ++mt) v.emplace_back((double)mt / (double)ln, (mt << 8) | ln);   // the divide of nw_code_values
  std::sort(v.begin(), v.end());
  memset(rank_out, 0, 65536 * sizeof(uint16_t));
  int rank = -1;
  double prev = -1.0;
  for (const auto &e : v) {
    if (e.first != prev) { ++rank; prev = e.first; }
    rank_out[e.second] = (uint16_t)rank;
  }
  if (distinct_out) *distinct_out = rank + 1;
  return DA_OK;
}

int da_similarity_nw_cross_topk(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues, const int64_t *y_offsets,
                                int64_t n, const char *matrix_name, int gap_open, int gap_ext, int top, int32_t *idx_out, double *val_out) {
  const int mid = da_matrix_id(matrix_name);             // before anything else, as in similarityNW
  if (mid < 0) return DA_ERR_BAD_MATRIX;
  if (m <= 0) return DA_OK;                              // no rows: nothing to write
  if (n <= 0) return fail(DA_ERR_BAD_ARG, "top must be in 1 .. n (got top = %d, n = 0)", top);
  NwCross c{x_residues, y_residues, x_offsets, y_offsets, m, n, mid, gap_open, gap_ext};
  int rc;
  if ((rc = c.check(idx_out != nullptr, [&] { return topk_check(top, n); }, "an order", 127,
                    "the NW top-k works on uint16 codes: sequences up to 127 residues")) != DA_OK || (rc = c.upload()) != DA_OK) return rc;
  const int64_t max_len = c.max_len;
  // equal values tie whatever their codes (2/4 and 3/6): the selection orders by the dense rank of a code's double value
  std::vector<uint16_t> ranks(65536);
  int distinct = 0;
  if ((rc = da_nw_code_ranks((int)max_len, ranks.data(), &distinct)) != DA_OK) return rc;
  DevBuf drank, didx, dkey;
  if ((rc = drank.alloc(65536 * sizeof(uint16_t))) != DA_OK || (rc = didx.alloc((size_t)m * (size_t)top * sizeof(int32_t))) != DA_OK ||
      (rc = dkey.alloc((size_t)m * (size_t)top * sizeof(uint16_t))) != DA_OK) return rc;
  DA_HIP_TRY(hipMemcpy(drank.p, ranks.data(), 65536 * sizeof(uint16_t), hipMemcpyHostToDevice));
  rc = topk_blocks(m, n, drank.as<uint16_t>(), bits_of(distinct - 1), top, didx.as<int32_t>(), top, dkey.as<uint16_t>(), top, nullptr,
                   [&](int64_t b0, int64_t b1, void *d, int64_t ld) { return c.rows(b0, b1, DA_OUT_COMPACT, d, ld, nullptr); });
  if (rc != DA_OK) return rc;
  return topk_to_host(didx, dkey, m, top, nw_code_values(65536, 0.0), idx_out, val_out);
}


// ---- one set, nearest-neighbour lists on the host boundary: row i lists the `top` columns j != i of the square matrix (dynaalign.h) -------------
int da_similarity_mh_knn(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, int n_hash, const uint32_t *seeds, int top,
                         int32_t *idx_out, double *val_out) {
  int rc = validate_mh(n, k, n_hash);                    // the checks of da_similarity_mh, in its order
  if (rc != DA_OK) return rc;
  if (!residues || !seeds || !idx_out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  int64_t total, max_len;
  if ((rc = check_offsets(offsets, n, &total, &max_len)) != DA_OK) return rc;
  if ((rc = knn_check(top, n)) != DA_OK) return rc;
  if (n_hash > 65535) return fail(DA_ERR_UNSUPPORTED, "the compare kernel counts in 16 bits: n_hash <= 65535 (got %d)", n_hash);
  if (n > 0x7ffffff0LL) return fail(DA_ERR_UNSUPPORTED, "nearest-neighbour lists: too many sequences");
  if ((rc = require_device()) != DA_OK) return rc;
  DeviceInput in;
  DevBuf didx, dkey;
  if ((rc = in.upload(residues, offsets, n, total, seeds, n_hash)) != DA_OK) return rc;
  if ((rc = didx.alloc((size_t)n * (size_t)top * sizeof(int32_t))) != DA_OK || (rc = dkey.alloc((size_t)n * (size_t)top * sizeof(uint16_t))) != DA_OK) return rc;
  if ((rc = mh_knn_lists(in.res.as<uint8_t>(), in.off.as<int64_t>(), n, k, n_hash, in.seeds.as<uint32_t>(), top, didx.as<int32_t>(), top,
                         dkey.as<uint16_t>(), top, nullptr)) != DA_OK) return rc;
  return topk_to_host(didx, dkey, n, top, mh_code_values(n_hash), idx_out, val_out);
}

int da_similarity_nw_knn(const uint8_t *residues, const int64_t *offsets, int64_t n, const char *matrix_name, int gap_open, int gap_ext, int top,
                         int32_t *idx_out, double *val_out, double *diag_out) {
  const int mid = da_matrix_id(matrix_name);             // before anything else, as in similarityNW
  if (mid < 0) return DA_ERR_BAD_MATRIX;
  if (!residues || !idx_out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  int rc;
  if ((rc = knn_check(top, n)) != DA_OK) return rc;      // where da_similarity_nw_edges checks n >= 2 and thresh_p
  int64_t total, max_len;
  if ((rc = check_offsets(offsets, n, &total, &max_len)) != DA_OK) return rc;
  if ((rc = nw_validate(residues, offsets, n)) != DA_OK) return rc;
  for (int64_t i = 0; i < n; ++i)
    if (offsets[i + 1] == offsets[i])
      return fail(DA_ERR_UNSUPPORTED, "sequence %lld is empty: its similarities are 0/0 = NaN and a NaN has no place in an order", (long long)(i + 1));
  if (max_len > 127) return fail(DA_ERR_UNSUPPORTED, "the NW nearest-neighbour lists work on uint16 codes: sequences up to 127 residues");
  if ((rc = require_device()) != DA_OK) return rc;
  NwCodes nw;
  if ((rc = nw.upload(residues, offsets, n, total)) != DA_OK) return rc;
  // equal values tie whatever their codes (2/4 and 3/6): the selection orders by the dense rank of a code's double value
  std::vector<uint16_t> ranks(65536);
  int distinct = 0;
  if ((rc = da_nw_code_ranks((int)max_len, ranks.data(), &distinct)) != DA_OK) return rc;
  DevBuf drank, didx, dkey, dself;
  if ((rc = drank.alloc(65536 * sizeof(uint16_t))) != DA_OK || (rc = didx.alloc((size_t)n * (size_t)top * sizeof(int32_t))) != DA_OK ||
      (rc = dkey.alloc((size_t)n * (size_t)top * sizeof(uint16_t))) != DA_OK || (rc = dself.alloc((size_t)n * sizeof(uint16_t))) != DA_OK) return rc;
  DA_HIP_TRY(hipMemcpy(drank.p, ranks.data(), 65536 * sizeof(uint16_t), hipMemcpyHostToDevice));
  // on ONE code buffer pair (p, q) is calc(seq[min(p, q)], seq[max(p, q)]): rows [b0, b1) x columns [0, n) are rows of the mirrored square matrix
  rc = topk_blocks(n, n, drank.as<uint16_t>(), bits_of(distinct - 1), top, didx.as<int32_t>(), top, dkey.as<uint16_t>(), top, nullptr,
                   [&](int64_t b0, int64_t b1, void *d, int64_t ld) {
                     return launch_nw_rect(nw.codes.as<uint8_t>(), nw.in.off.as<int64_t>(), n, max_len, mid, gap_open, gap_ext, b0, b1, 0, n, DA_OUT_COMPACT,
                                           d, ld, nullptr);
                   }, true, dself.as<uint16_t>());
  if (rc != DA_OK) return rc;
  const std::vector<double> table = nw_code_values(65536, 0.0);
  if (diag_out) {
    std::vector<uint16_t> sk((size_t)n);
    DA_HIP_TRY(hipMemcpy(sk.data(), dself.p, (size_t)n * sizeof(uint16_t), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i) diag_out[i] = table[sk[(size_t)i]];
  }
  return topk_to_host(didx, dkey, n, top, table, idx_out, val_out);
}

// ---- the exact Jaccard index of k-shingle sets on the host boundary (dynaalign.h) ----------------------------------------------------------------
// What every host call shares.  check_one / check_two: the documented validation of one set / of x then y, before a device is needed.  build():
// DA_ERR_NO_DEVICE last, then the sequences -- two sets as ONE operand [x ; y] of m + n sequences, like NwCross -- and their sorted distinct keys
// (k_jaccard_sets) on the device.  rect(): rows x columns of that operand as uint16 codes (intersection << 8 | union) or doubles.
// JaccardSets(1024) is the operand of the _long calls: the same checks with its limit in the texts, uint16 counts, the long kernels, and
// rect() as DA_OUT_PACK32 codes (intersection << 16 | union) or doubles.
struct JaccardSets {
  const int limit;                                       // shingle positions per sequence: 127, or 1024 (the long kernels)
  explicit JaccardSets(int limit_ = 127) : limit(limit_) {}
  bool is_long() const { return limit > 127; }
  int k = 0;
  int64_t m = 0, n = 0;                                  // one set: m == 0, n sequences; two sets: x has m, y has n
  int64_t x_total = 0, y_total = 0, max_len = 0, ld_keys = 0;
  DeviceInput in;
  DevBuf keys, counts;
  int lengths(const int64_t *off, int64_t cnt, int k) const {
    for (int64_t i = 0; i < cnt; ++i) {
      const int rc = off[i + 1] - off[i] - k + 1 > limit ? jaccard_limits(k, off[i + 1] - off[i], i + 1, limit) : DA_OK;
      if (rc != DA_OK) return rc;
    }
    return DA_OK;
  }
  int check_one(const uint8_t *res, const int64_t *off, int64_t n_, int k_, bool out_ok) {
    if (n_ <= 0) return fail(DA_ERR_EMPTY_INPUT, "%s", da_status_message(DA_ERR_EMPTY_INPUT));
    if (k_ <= 0) return fail(DA_ERR_BAD_K, "%s", da_status_message(DA_ERR_BAD_K));
    if (!res || !out_ok) return fail(DA_ERR_BAD_ARG, "NULL pointer");
    int rc;
    if ((rc = check_offsets(off, n_, &y_total, &max_len)) != DA_OK) return rc;
    if ((rc = jaccard_limits(k_, 0, 0)) != DA_OK || (rc = lengths(off, n_, k_)) != DA_OK) return rc;
    if (n_ > 0x7ffffff0LL) return fail(DA_ERR_UNSUPPORTED, "exact Jaccard: too many sequences");
    k = k_; m = 0; n = n_;
    return DA_OK;
  }
  // (k and the empty shapes are the caller's: they differ between the two-set calls)
  int check_two(const uint8_t *xr, const int64_t *xo, int64_t m_, const uint8_t *yr, const int64_t *yo, int64_t n_, int k_, bool out_ok) {
    if (!xr || !yr || !out_ok) return fail(DA_ERR_BAD_ARG, "NULL pointer");
    int64_t x_max, y_max;
    int rc;
    if ((rc = check_offsets(xo, m_, &x_total, &x_max)) != DA_OK || (rc = check_offsets(yo, n_, &y_total, &y_max)) != DA_OK) return rc;
    if ((rc = jaccard_limits(k_, 0, 0)) != DA_OK || (rc = lengths(xo, m_, k_)) != DA_OK || (rc = lengths(yo, n_, k_)) != DA_OK) return rc;
    if (m_ + n_ > 0x7ffffff0LL) return fail(DA_ERR_UNSUPPORTED, "exact Jaccard: too many sequences");
    max_len = std::max(x_max, y_max);
    k = k_; m = m_; n = n_;
    return DA_OK;
  }
  int sets() {
    int rc;
    ld_keys = jaccard_sets_ld(max_len, k);
    if ((rc = keys.alloc((size_t)(m + n) * (size_t)ld_keys * (k <= 4 ? 4 : 8))) != DA_OK ||
        (rc = counts.alloc((size_t)(m + n) * (is_long() ? sizeof(uint16_t) : 1))) != DA_OK) return rc;
    if (is_long())
      return launch_jaccard_sets_long(in.res.as<uint8_t>(), in.off.as<int64_t>(), m + n, max_len, k, keys.p, ld_keys, counts.as<uint16_t>(), nullptr);
    return launch_jaccard_sets(in.res.as<uint8_t>(), in.off.as<int64_t>(), m + n, max_len, k, keys.p, ld_keys, counts.as<uint8_t>(), nullptr);
  }
  int build(const uint8_t *res, const int64_t *off) {
    int rc;
    if ((rc = require_device()) != DA_OK || (rc = in.upload(res, off, n, y_total, nullptr, 0)) != DA_OK) return rc;
    return sets();
  }
  int build(const uint8_t *xr, const int64_t *xo, const uint8_t *yr, const int64_t *yo) {
    int rc;
    if ((rc = require_device()) != DA_OK) return rc;
    std::vector<uint8_t> res((size_t)(x_total + y_total) + 1);
    std::vector<int64_t> off((size_t)(m + n) + 1);
    if (x_total) memcpy(res.data(), xr, (size_t)x_total);
    if (y_total) memcpy(res.data() + x_total, yr, (size_t)y_total);
    for (int64_t i = 0; i <= m; ++i) off[(size_t)i] = xo[i];
    for (int64_t j = 1; j <= n; ++j) off[(size_t)(m + j)] = x_total + yo[j];
    if ((rc = in.upload(res.data(), off.data(), m + n, x_total + y_total, nullptr, 0)) != DA_OK) return rc;
    return sets();
  }
  int rect(int64_t r0, int64_t r1, int64_t c0, int64_t c1, int kind, void *d, int64_t ld, hipStream_t stream) const {
    if (is_long()) return launch_jaccard_rect_long(keys.p, counts.as<uint16_t>(), m + n, ld_keys, k, r0, r1, c0, c1, kind, d, ld, stream);
    return launch_jaccard_rect(keys.p, counts.as<uint8_t>(), m + n, ld_keys, k, r0, r1, c0, c1, kind, d, ld, stream);
  }
  // the largest shingle count of the call (at least 1: the code of two empty sets is 1 << 8 | 1) and the bins its uint16 codes fall into
  int shingles() const { return (int)std::max<int64_t>(1, max_len - k + 1); }
  int nbins() const {
    const int64_t sh = shingles();
    return (int)((sh << 8) | (2 * sh)) + 1;
  }
};

// the rank table of the codes (equal values tie whatever their codes) on the device; *bits_out: the bits a rank takes
static int jaccard_ranks(DevBuf &drank, int *bits_out) {
  std::vector<uint16_t> ranks(65536);
  int distinct = 0, rc;
  if ((rc = da_nw_code_ranks(127, ranks.data(), &distinct)) != DA_OK || (rc = drank.alloc(65536 * sizeof(uint16_t))) != DA_OK) return rc;
  DA_HIP_TRY(hipMemcpy(drank.p, ranks.data(), 65536 * sizeof(uint16_t), hipMemcpyHostToDevice));
  *bits_out = bits_of(distinct - 1);
  return DA_OK;
}

int da_similarity_jaccard(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, double *out) {
  JaccardSets js;
  int rc;
  if ((rc = js.check_one(residues, offsets, n, k, out != nullptr)) != DA_OK || (rc = js.build(residues, offsets)) != DA_OK) return rc;
  Trace tr("similarityJaccard host path");
  const std::vector<double> table = nw_code_values(65536, 0.0);
  if (rows_per_block(n, sizeof(uint16_t)) >= n)
    return codes_to_host(n, out, table, tr, [&](void *d) { return js.rect(0, n, 0, n, DA_OUT_COMPACT, d, n, nullptr); });
  return rows_to_host(n, 0, n, sizeof(uint16_t), out, [&](int64_t b0, int64_t b1, void *d) { return js.rect(b0, b1, 0, n, DA_OUT_COMPACT, d, n, nullptr); },
                      nullptr, nullptr, table.data());
}

int da_similarity_jaccard_cross(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues, const int64_t *y_offsets,
                                int64_t n, int k, double *out, int column_major) {
  if (k <= 0) return fail(DA_ERR_BAD_K, "%s", da_status_message(DA_ERR_BAD_K));
  if (m <= 0 || n <= 0) return DA_OK;                    // an m x 0 or 0 x n matrix: nothing to write
  JaccardSets js;
  int rc;
  if ((rc = js.check_two(x_residues, x_offsets, m, y_residues, y_offsets, n, k, out != nullptr)) != DA_OK ||
      (rc = js.build(x_residues, x_offsets, y_residues, y_offsets)) != DA_OK) return rc;
  const int64_t rows = column_major ? n : m, cols = column_major ? m : n;
  const std::vector<double> table = nw_code_values(65536, 0.0);
  // J is symmetric: rows of y against columns of x are the transpose, R's column-major NumericMatrix(m, n)
  return rows_to_host(cols, 0, rows, sizeof(uint16_t), out, [&](int64_t b0, int64_t b1, void *d) {
    return column_major ? js.rect(m + b0, m + b1, 0, m, DA_OUT_COMPACT, d, cols, nullptr) : js.rect(b0, b1, m, m + n, DA_OUT_COMPACT, d, cols, nullptr);
  }, nullptr, nullptr, table.data());
}

int da_similarity_jaccard_cross_topk(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues, const int64_t *y_offsets,
                                     int64_t n, int k, int top, int32_t *idx_out, double *val_out) {
  if (k <= 0) return fail(DA_ERR_BAD_K, "%s", da_status_message(DA_ERR_BAD_K));
  if (m <= 0) return DA_OK;                              // no rows: nothing to write
  if (n <= 0) return fail(DA_ERR_BAD_ARG, "top must be in 1 .. n (got top = %d, n = 0)", top);
  JaccardSets js;
  int rc, bits = 16;
  if ((rc = js.check_two(x_residues, x_offsets, m, y_residues, y_offsets, n, k, idx_out != nullptr)) != DA_OK || (rc = topk_check(top, n)) != DA_OK ||
      (rc = js.build(x_residues, x_offsets, y_residues, y_offsets)) != DA_OK) return rc;
  DevBuf drank, didx, dkey;
  if ((rc = jaccard_ranks(drank, &bits)) != DA_OK || (rc = didx.alloc((size_t)m * (size_t)top * sizeof(int32_t))) != DA_OK ||
      (rc = dkey.alloc((size_t)m * (size_t)top * sizeof(uint16_t))) != DA_OK) return rc;
  rc = topk_blocks(m, n, drank.as<uint16_t>(), bits, top, didx.as<int32_t>(), top, dkey.as<uint16_t>(), top, nullptr,
                   [&](int64_t b0, int64_t b1, void *d, int64_t ld) { return js.rect(b0, b1, m, m + n, DA_OUT_COMPACT, d, ld, nullptr); });
  if (rc != DA_OK) return rc;
  return topk_to_host(didx, dkey, m, top, nw_code_values(65536, 0.0), idx_out, val_out);
}

int da_similarity_jaccard_knn(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, int top, int32_t *idx_out, double *val_out) {
  JaccardSets js;
  int rc, bits = 16;
  if ((rc = js.check_one(residues, offsets, n, k, idx_out != nullptr)) != DA_OK || (rc = knn_check(top, n)) != DA_OK ||
      (rc = js.build(residues, offsets)) != DA_OK) return rc;
  DevBuf drank, didx, dkey;
  if ((rc = jaccard_ranks(drank, &bits)) != DA_OK || (rc = didx.alloc((size_t)n * (size_t)top * sizeof(int32_t))) != DA_OK ||
      (rc = dkey.alloc((size_t)n * (size_t)top * sizeof(uint16_t))) != DA_OK) return rc;
  rc = topk_blocks(n, n, drank.as<uint16_t>(), bits, top, didx.as<int32_t>(), top, dkey.as<uint16_t>(), top, nullptr,
                   [&](int64_t b0, int64_t b1, void *d, int64_t ld) { return js.rect(b0, b1, 0, n, DA_OUT_COMPACT, d, ld, nullptr); }, true);
  if (rc != DA_OK) return rc;
  return topk_to_host(didx, dkey, n, top, nw_code_values(65536, 0.0), idx_out, val_out);
}

// the exact index + clusterbreak's threshold step as an edge list: the codes have the NW code's shape, so its histogram / quantile / extraction
// path applies with the same value table
static int jaccard_edges_core(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, double thresh_p, bool want_edges, EdgeSet &es,
                              int64_t *n_edges_out) {
  JaccardSets js;
  int rc;
  if ((rc = js.check_one(residues, offsets, n, k, true)) != DA_OK) return rc;
  if (n < 2) return fail(DA_ERR_BAD_ARG, "the threshold is a quantile of the strict upper triangle: need >= 2 sequences");
  if (!(thresh_p >= 0.0 && thresh_p <= 1.0)) return fail(DA_ERR_BAD_ARG, "thresh_p must be in [0, 1]");
  if ((rc = js.build(residues, offsets)) != DA_OK) return rc;
  DevBuf cnt, hist;
  const int nbins = js.nbins();
  if ((rc = cnt.alloc((size_t)n * (size_t)n * 2)) != DA_OK || (rc = hist.alloc((size_t)nbins * 8)) != DA_OK) return rc;   // uint16 codes stay on the device
  DA_HIP_TRY(hipMemset(hist.p, 0, (size_t)nbins * 8));
  if ((rc = js.rect(0, n, 0, n, DA_OUT_COMPACT, cnt.p, n, nullptr)) != DA_OK) return rc;
  if ((rc = launch_upper_histogram(cnt.as<uint16_t>(), n, n, nbins, hist.as<unsigned long long>(), nullptr)) != DA_OK) return rc;
  return edges_from_counts(cnt.as<uint16_t>(), n, nbins, hist.as<unsigned long long>(), nw_code_values(nbins, 0.0), thresh_p, want_edges, es, n_edges_out);
}

int da_similarity_jaccard_edges(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, double thresh_p, double *threshold_out,
                                int64_t *n_edges_out, int64_t capacity, int32_t *ei, int32_t *ej, double *ew) {
  return edges_run_deliver(threshold_out, n_edges_out, capacity, ei, ej, ew, [&](bool want_edges, EdgeSet &es, int64_t *cnt) {
    return jaccard_edges_core(residues, offsets, n, k, thresh_p, want_edges, es, cnt);
  });
}

int da_similarity_jaccard_edges_begin(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, double thresh_p, da_edges **handle_out,
                                      double *threshold_out, int64_t *n_edges_out) {
  return edges_run_handle(handle_out, threshold_out, n_edges_out, [&](bool want_edges, EdgeSet &es, int64_t *cnt) {
    return jaccard_edges_core(residues, offsets, n, k, thresh_p, want_edges, es, cnt);
  });
}

// ---- the alignment PATH of listed pairs (nw_align_kernels.hip): which residue sits opposite which, and where the gaps are -------------------
size_t da_nw_align_workspace_bytes(int64_t pairs) { return nw_align_workspace_bytes(pairs); }

int da_dev_nw_align_pairs(const uint8_t *d_x_codes, const int64_t *d_x_offsets, int64_t m, const uint8_t *d_y_codes, const int64_t *d_y_offsets,
                          int64_t n, const int32_t *d_pair_x, const int32_t *d_pair_y, int64_t pairs, int matrix_id, int gap_open, int gap_ext,
                          uint8_t *d_ops, int64_t ld_ops, int32_t *d_len, int32_t *d_matches, int32_t *d_score, void *d_work, size_t work_bytes,
                          void *stream) {
  if (pairs < 0 || m < 0 || n < 0) return fail(DA_ERR_BAD_ARG, "negative count");
  if (pairs == 0) return DA_OK;
  if ((d_pair_x == nullptr) != (d_pair_y == nullptr)) return fail(DA_ERR_BAD_ARG, "pair_x and pair_y must both be given or both be NULL");
  if (!d_pair_x && (m != pairs || n != pairs)) return fail(DA_ERR_BAD_ARG, "without pair lists pair p is x[p] against y[p]: m == n == pairs");
  if (!d_x_codes || !d_x_offsets || !d_y_codes || !d_y_offsets) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (d_ops && ld_ops < 0) return fail(DA_ERR_BAD_ARG, "negative ld_ops");
  int rc;
  if ((rc = require_device()) != DA_OK) return rc;
  return launch_nw_align(d_x_codes, d_x_offsets, m, d_y_codes, d_y_offsets, n, d_pair_x, d_pair_y, 0, pairs, matrix_id, gap_open, gap_ext, d_ops, ld_ops,
                         d_len, d_matches, d_score, d_work, work_bytes, static_cast<hipStream_t>(stream));
}

// What the reference's lazy fill would raise first with the listed pairs visited p ascending, each in calc's own order (src/pairwiseSeqAlign.cpp:
// 238-250: sequence1[0], every character of sequence2, then sequence1[1], ...; an empty sequence1 checks nothing, an empty sequence2 still has all
// of sequence1 checked).  first_bad(set)[i]: position of the first invalid byte of sequence i, -1 if none.
static std::vector<int32_t> nw_first_bad(const uint8_t *res, const int64_t *off, int64_t count) {
  static const char order[] = "ARNDCQEGHILKMFPSTWYVBZX*";
  std::vector<int32_t> bad((size_t)count, -1);
  for (int64_t i = 0; i < count; ++i)
    for (int64_t p = off[i]; p < off[i + 1]; ++p)
      if (res[p] == 0 || strchr(order, res[p]) == nullptr) { bad[(size_t)i] = (int32_t)std::min<int64_t>(p - off[i], INT32_MAX); break; }
  return bad;
}

// Everything da_nw_align_pairs and da_nw_align_long_pairs check before a device is needed, in the documented order; they differ in the longest
// sequence they take.  *nothing: pairs == 0 (DA_OK, nothing to write).
static int nw_align_validate(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues, const int64_t *y_offsets,
                             int64_t n, const int32_t *pair_x, const int32_t *pair_y, int64_t pairs, const char *matrix_name, const uint8_t *ops_out,
                             int64_t ld_ops, int max_residues, int *mid_out, int64_t *x_total, int64_t *y_total, bool *nothing) {
  *nothing = false;
  const int mid = da_matrix_id(matrix_name);             // before anything else, as in similarityNW
  if (mid < 0) return DA_ERR_BAD_MATRIX;
  *mid_out = mid;
  if (pairs == 0) { *nothing = true; return DA_OK; }     // nothing listed: nothing to write
  if (pairs < 0 || m < 0 || n < 0) return fail(DA_ERR_BAD_ARG, "negative count");
  if ((pair_x == nullptr) != (pair_y == nullptr)) return fail(DA_ERR_BAD_ARG, "pair_x and pair_y must both be given or both be NULL");
  if (!pair_x && (m != pairs || n != pairs)) return fail(DA_ERR_BAD_ARG, "without pair lists pair p is x[p] against y[p]: m == n == pairs");
  if (!x_residues || !y_residues) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  int64_t x_max, y_max;
  int rc;
  if ((rc = check_offsets(x_offsets, m, x_total, &x_max)) != DA_OK || (rc = check_offsets(y_offsets, n, y_total, &y_max)) != DA_OK) return rc;
  auto xi = [&](int64_t p) { return pair_x ? (int64_t)pair_x[p] : p; };
  auto yj = [&](int64_t p) { return pair_y ? (int64_t)pair_y[p] : p; };
  for (int64_t p = 0; p < pairs; ++p) {
    if (xi(p) < 0 || xi(p) >= m) return fail(DA_ERR_BAD_ARG, "pair %lld: index %lld is outside x (m = %lld)", (long long)p, (long long)xi(p), (long long)m);
    if (yj(p) < 0 || yj(p) >= n) return fail(DA_ERR_BAD_ARG, "pair %lld: index %lld is outside y (n = %lld)", (long long)p, (long long)yj(p), (long long)n);
  }
  int64_t need = 0;
  for (int64_t p = 0; p < pairs; ++p) {
    const int64_t lx = x_offsets[xi(p) + 1] - x_offsets[xi(p)], ly = y_offsets[yj(p) + 1] - y_offsets[yj(p)];
    if (lx > max_residues || ly > max_residues)
      return fail(DA_ERR_UNSUPPORTED, "the alignment kernel takes sequences up to %d residues (pair %lld: %lld and %lld)", max_residues, (long long)p,
                  (long long)lx, (long long)ly);
    need = std::max(need, lx + ly);
  }
  if (ops_out && ld_ops < need)
    return fail(DA_ERR_BAD_ARG, "ld_ops = %lld is smaller than the longest listed len(x) + len(y) = %lld", (long long)ld_ops, (long long)need);
  const std::vector<int32_t> bx = nw_first_bad(x_residues, x_offsets, m), by = nw_first_bad(y_residues, y_offsets, n);
  for (int64_t p = 0; p < pairs; ++p) {
    const int64_t i = xi(p), j = yj(p);
    if (x_offsets[i + 1] == x_offsets[i]) continue;                                   // no row runs
    const uint8_t *s1 = x_residues + x_offsets[i], *s2 = y_residues + y_offsets[j];
    if (bx[(size_t)i] == 0) return fail(DA_ERR_BAD_RESIDUE_SEQ1, "Invalid amino acid in sequence1: %c", (char)s1[0]);
    if (by[(size_t)j] >= 0) return fail(DA_ERR_BAD_RESIDUE_SEQ2, "Invalid amino acid in sequence2: %c", (char)s2[by[(size_t)j]]);
    if (bx[(size_t)i] > 0) return fail(DA_ERR_BAD_RESIDUE_SEQ1, "Invalid amino acid in sequence1: %c", (char)s1[bx[(size_t)i]]);
  }
  return DA_OK;
}

int da_nw_align_pairs(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues, const int64_t *y_offsets, int64_t n,
                      const int32_t *pair_x, const int32_t *pair_y, int64_t pairs, const char *matrix_name, int gap_open, int gap_ext,
                      uint8_t *ops_out, int64_t ld_ops, int32_t *len_out, int32_t *matches_out, int32_t *score_out) {
  int mid = 0, rc;
  int64_t x_total = 0, y_total = 0;
  bool nothing = false;
  if ((rc = nw_align_validate(x_residues, x_offsets, m, y_residues, y_offsets, n, pair_x, pair_y, pairs, matrix_name, ops_out, ld_ops, 127, &mid,
                              &x_total, &y_total, &nothing)) != DA_OK || nothing) return rc;
  if ((rc = require_device()) != DA_OK) return rc;
  NwCodes nx, ny;
  if ((rc = nx.upload(x_residues, x_offsets, m, x_total)) != DA_OK || (rc = ny.upload(y_residues, y_offsets, n, y_total)) != DA_OK) return rc;
  DevBuf dpx, dpy, dlen, dmt, dsc, dops, work;
  const size_t ibytes = (size_t)pairs * sizeof(int32_t);
  if (pair_x) {
    if ((rc = dpx.alloc(ibytes)) != DA_OK || (rc = dpy.alloc(ibytes)) != DA_OK) return rc;
    DA_HIP_TRY(hipMemcpy(dpx.p, pair_x, ibytes, hipMemcpyHostToDevice));
    DA_HIP_TRY(hipMemcpy(dpy.p, pair_y, ibytes, hipMemcpyHostToDevice));
  }
  if ((rc = dlen.alloc(ibytes)) != DA_OK || (rc = dmt.alloc(ibytes)) != DA_OK || (rc = dsc.alloc(ibytes)) != DA_OK) return rc;
  // blocks of pairs: workspace + ops bytes of a block within DYNAALIGN_BLOCK_BYTES (half of the free memory without it), at most 2^19 pairs
  const size_t per_pair = nw_align_workspace_bytes(64) / 64 + (ops_out ? (size_t)ld_ops : 0);
  const int64_t blk = std::min<int64_t>(std::min<int64_t>(block_rows(1, per_pair), (int64_t)1 << 19), ceil_div(pairs, 64) * 64);
  const size_t wbytes = nw_align_workspace_bytes(blk);
  if ((rc = work.alloc(wbytes)) != DA_OK) return rc;
  if (ops_out && (rc = dops.alloc((size_t)blk * (size_t)ld_ops)) != DA_OK) return rc;
  for (int64_t b0 = 0; b0 < pairs; b0 += blk) {
    const int64_t cnt = std::min(blk, pairs - b0);
    rc = launch_nw_align(nx.codes.as<uint8_t>(), nx.in.off.as<int64_t>(), m, ny.codes.as<uint8_t>(), ny.in.off.as<int64_t>(), n,
                         pair_x ? dpx.as<int32_t>() + b0 : nullptr, pair_x ? dpy.as<int32_t>() + b0 : nullptr, b0, cnt, mid, gap_open, gap_ext,
                         ops_out ? dops.as<uint8_t>() : nullptr, ld_ops, dlen.as<int32_t>() + b0, dmt.as<int32_t>() + b0, dsc.as<int32_t>() + b0, work.p,
                         wbytes, nullptr);
    if (rc != DA_OK) return rc;
    if (ops_out) DA_HIP_TRY(hipMemcpy(ops_out + (size_t)b0 * (size_t)ld_ops, dops.p, (size_t)cnt * (size_t)ld_ops, hipMemcpyDeviceToHost));
  }
  if (len_out) DA_HIP_TRY(hipMemcpy(len_out, dlen.p, ibytes, hipMemcpyDeviceToHost));
  if (matches_out) DA_HIP_TRY(hipMemcpy(matches_out, dmt.p, ibytes, hipMemcpyDeviceToHost));
  if (score_out) DA_HIP_TRY(hipMemcpy(score_out, dsc.p, ibytes, hipMemcpyDeviceToHost));
  return sync_or_fail("the alignment kernel failed");
}

// ---- the same for sequences of up to 1024 residues (nw_align_long_kernels.hip): one wavefront per pair --------------------------------------
size_t da_nw_align_long_workspace_bytes(int64_t pairs, int64_t max_len) { return nw_align_long_workspace_bytes(pairs, max_len); }

int da_dev_nw_align_long_pairs(const uint8_t *d_x_codes, const int64_t *d_x_offsets, int64_t m, const uint8_t *d_y_codes, const int64_t *d_y_offsets,
                               int64_t n, const int32_t *d_pair_x, const int32_t *d_pair_y, int64_t pairs, int matrix_id, int gap_open, int gap_ext,
                               uint8_t *d_ops, int64_t ld_ops, int32_t *d_len, int32_t *d_matches, int32_t *d_score, int64_t max_len, void *d_work,
                               size_t work_bytes, void *stream) {
  if (pairs < 0 || m < 0 || n < 0) return fail(DA_ERR_BAD_ARG, "negative count");
  if (pairs == 0) return DA_OK;
  if ((d_pair_x == nullptr) != (d_pair_y == nullptr)) return fail(DA_ERR_BAD_ARG, "pair_x and pair_y must both be given or both be NULL");
  if (!d_pair_x && (m != pairs || n != pairs)) return fail(DA_ERR_BAD_ARG, "without pair lists pair p is x[p] against y[p]: m == n == pairs");
  if (!d_x_codes || !d_x_offsets || !d_y_codes || !d_y_offsets) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (d_ops && ld_ops < 0) return fail(DA_ERR_BAD_ARG, "negative ld_ops");
  if (max_len < 0) return fail(DA_ERR_BAD_ARG, "negative max_len");
  if (d_ops && (!d_work || work_bytes < nw_align_long_slot_bytes(max_len)))
    return fail(DA_ERR_BAD_ARG, "the alignment workspace holds less than one slot of (max_len + 63) * 256 bytes (%zu bytes; da_nw_align_long_workspace_bytes)",
                d_work ? work_bytes : (size_t)0);
  int rc;
  if ((rc = require_device()) != DA_OK) return rc;
  return launch_nw_align_long(d_x_codes, d_x_offsets, m, d_y_codes, d_y_offsets, n, d_pair_x, d_pair_y, 0, pairs, matrix_id, gap_open, gap_ext, d_ops,
                              ld_ops, d_len, d_matches, d_score, max_len, d_work, work_bytes, static_cast<hipStream_t>(stream));
}

int da_nw_align_long_pairs(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues, const int64_t *y_offsets,
                           int64_t n, const int32_t *pair_x, const int32_t *pair_y, int64_t pairs, const char *matrix_name, int gap_open, int gap_ext,
                           uint8_t *ops_out, int64_t ld_ops, int32_t *len_out, int32_t *matches_out, int32_t *score_out) {
  int mid = 0, rc;
  int64_t x_total = 0, y_total = 0;
  bool nothing = false;
  if ((rc = nw_align_validate(x_residues, x_offsets, m, y_residues, y_offsets, n, pair_x, pair_y, pairs, matrix_name, ops_out, ld_ops, 1024, &mid,
                              &x_total, &y_total, &nothing)) != DA_OK || nothing) return rc;
  if ((rc = require_device()) != DA_OK) return rc;
  NwCodes nx, ny;
  if ((rc = nx.upload(x_residues, x_offsets, m, x_total)) != DA_OK || (rc = ny.upload(y_residues, y_offsets, n, y_total)) != DA_OK) return rc;
  // the split: pairs with both sequences within the lane-per-pair kernels' 127 residues go there, every other pair takes a wavefront
  struct Group { std::vector<int32_t> px, py; std::vector<int64_t> at; };
  Group g[2];                                              // 0 short, 1 long
  int64_t long_max = 0;
  for (int64_t p = 0; p < pairs; ++p) {
    const int64_t i = pair_x ? (int64_t)pair_x[p] : p, j = pair_y ? (int64_t)pair_y[p] : p;
    const int64_t lx = x_offsets[i + 1] - x_offsets[i], ly = y_offsets[j + 1] - y_offsets[j];
    Group &t = g[lx > 127 || ly > 127];
    if (&t == &g[1]) long_max = std::max(long_max, std::max(lx, ly));
    t.px.push_back((int32_t)i); t.py.push_back((int32_t)j); t.at.push_back(p);
  }
  const size_t budget = block_budget();                    // DYNAALIGN_BLOCK_BYTES, or half of the free memory
  std::vector<uint8_t> stage;
  std::vector<int32_t> ibuf;
  for (int k = 0; k < 2; ++k) {
    const int64_t cnt_k = (int64_t)g[k].at.size();
    if (cnt_k == 0) continue;
    const bool whole = cnt_k == pairs;                     // the listed order is the group's order: results go straight to the caller
    DevBuf dpx, dpy, dlen, dmt, dsc, dops, work;
    const size_t ibytes = (size_t)cnt_k * sizeof(int32_t);
    if ((rc = dpx.alloc(ibytes)) != DA_OK || (rc = dpy.alloc(ibytes)) != DA_OK || (rc = dlen.alloc(ibytes)) != DA_OK ||
        (rc = dmt.alloc(ibytes)) != DA_OK || (rc = dsc.alloc(ibytes)) != DA_OK) return rc;
    DA_HIP_TRY(hipMemcpy(dpx.p, g[k].px.data(), ibytes, hipMemcpyHostToDevice));
    DA_HIP_TRY(hipMemcpy(dpy.p, g[k].py.data(), ibytes, hipMemcpyHostToDevice));
    // blocks of pairs, as in da_nw_align_pairs: ops rows (and the short kernels' per-pair workspace) of a block within the budget.  The
    // wavefront kernel's workspace does not grow with the pairs: as many slots as fit half of the budget, at least one.
    int64_t blk;
    size_t wbytes = 0;
    if (k == 0) {
      const size_t per_pair = nw_align_workspace_bytes(64) / 64 + (ops_out ? (size_t)ld_ops : 0);
      blk = std::min<int64_t>(std::min<int64_t>(block_rows(1, per_pair), (int64_t)1 << 19), ceil_div(cnt_k, 64) * 64);
      wbytes = nw_align_workspace_bytes(blk);
    } else {
      blk = cnt_k;
      if (ops_out) {
        const size_t slot = nw_align_long_slot_bytes(long_max);
        const int64_t slots = std::max<int64_t>(1, std::min<int64_t>((int64_t)(budget / 2 / slot), cnt_k));
        wbytes = std::min(nw_align_long_workspace_bytes(cnt_k, long_max), (size_t)slots * slot);
        blk = std::min<int64_t>(std::min<int64_t>(block_rows(1, 2 * (size_t)std::max<int64_t>(ld_ops, 1)), (int64_t)1 << 19), cnt_k);
      }
    }
    if (wbytes && (rc = work.alloc(wbytes)) != DA_OK) return rc;
    if (ops_out && (rc = dops.alloc((size_t)blk * (size_t)ld_ops)) != DA_OK) return rc;
    for (int64_t b0 = 0; b0 < cnt_k; b0 += blk) {
      const int64_t cnt = std::min(blk, cnt_k - b0);
      if (k == 0)
        rc = launch_nw_align(nx.codes.as<uint8_t>(), nx.in.off.as<int64_t>(), m, ny.codes.as<uint8_t>(), ny.in.off.as<int64_t>(), n,
                             dpx.as<int32_t>() + b0, dpy.as<int32_t>() + b0, b0, cnt, mid, gap_open, gap_ext, ops_out ? dops.as<uint8_t>() : nullptr,
                             ld_ops, dlen.as<int32_t>() + b0, dmt.as<int32_t>() + b0, dsc.as<int32_t>() + b0, work.p, wbytes, nullptr);
      else
        rc = launch_nw_align_long(nx.codes.as<uint8_t>(), nx.in.off.as<int64_t>(), m, ny.codes.as<uint8_t>(), ny.in.off.as<int64_t>(), n,
                                  dpx.as<int32_t>() + b0, dpy.as<int32_t>() + b0, b0, cnt, mid, gap_open, gap_ext,
                                  ops_out ? dops.as<uint8_t>() : nullptr, ld_ops, dlen.as<int32_t>() + b0, dmt.as<int32_t>() + b0,
                                  dsc.as<int32_t>() + b0, long_max, work.p, wbytes, nullptr);
      if (rc != DA_OK) return rc;
      if (!ops_out) continue;
      if (whole) {
        DA_HIP_TRY(hipMemcpy(ops_out + (size_t)b0 * (size_t)ld_ops, dops.p, (size_t)cnt * (size_t)ld_ops, hipMemcpyDeviceToHost));
      } else {
        stage.resize((size_t)cnt * (size_t)ld_ops);
        DA_HIP_TRY(hipMemcpy(stage.data(), dops.p, stage.size(), hipMemcpyDeviceToHost));
        for (int64_t r = 0; r < cnt; ++r)
          memcpy(ops_out + (size_t)g[k].at[(size_t)(b0 + r)] * (size_t)ld_ops, stage.data() + (size_t)r * (size_t)ld_ops, (size_t)ld_ops);
      }
    }
    int32_t *outs[3] = {len_out, matches_out, score_out};
    DevBuf *src[3] = {&dlen, &dmt, &dsc};
    for (int f = 0; f < 3; ++f) {
      if (!outs[f]) continue;
      if (whole) { DA_HIP_TRY(hipMemcpy(outs[f], src[f]->p, ibytes, hipMemcpyDeviceToHost)); continue; }
      ibuf.resize((size_t)cnt_k);
      DA_HIP_TRY(hipMemcpy(ibuf.data(), src[f]->p, ibytes, hipMemcpyDeviceToHost));
      for (int64_t r = 0; r < cnt_k; ++r) outs[f][g[k].at[(size_t)r]] = ibuf[(size_t)r];
    }
    if ((rc = sync_or_fail("the alignment kernel failed")) != DA_OK) return rc;
  }
  return DA_OK;
}

// ---- the center-star consensus of clusters (consensus_kernels.hip) on top of the two alignment kernels ---------------------------------------
// the pooled table on the host: cluster_ptr[0] == 0, every cluster has a member, the last entry is the number of sequences
static int cons_table_check(const int64_t *cluster_ptr, int64_t n, int64_t clusters) {
  if (!cluster_ptr) return fail(DA_ERR_BAD_ARG, "cluster_ptr is NULL");
  if (cluster_ptr[0] != 0) return fail(DA_ERR_BAD_ARG, "cluster_ptr[0] must be 0");
  for (int64_t k = 0; k < clusters; ++k)
    if (cluster_ptr[k + 1] <= cluster_ptr[k]) return fail(DA_ERR_BAD_ARG, "cluster %lld has no member", (long long)k);
  if (cluster_ptr[clusters] != n) return fail(DA_ERR_BAD_ARG, "cluster_ptr ends at %lld, not at n = %lld", (long long)cluster_ptr[clusters], (long long)n);
  return DA_OK;
}

size_t da_dev_cluster_consensus_workspace_bytes(const int64_t *cluster_ptr, int64_t clusters, int64_t max_len, int minimal) {
  return cluster_consensus_workspace_bytes(cluster_ptr, clusters, max_len, minimal != 0);
}

int da_dev_cluster_consensus(const uint8_t *d_codes, const int64_t *d_offsets, int64_t n, const int64_t *cluster_ptr, const int64_t *d_cluster_ptr,
                             int64_t clusters, int64_t max_len, int matrix_id, int gap_open, int gap_ext, uint8_t *d_cons, int64_t ld_cons,
                             int32_t *d_cons_len, int32_t *d_center, void *d_work, size_t work_bytes, void *stream) {
  if (n < 0 || clusters < 0) return fail(DA_ERR_BAD_ARG, "negative count");
  if (clusters == 0) return n == 0 ? DA_OK : fail(DA_ERR_BAD_ARG, "no clusters for %lld sequences", (long long)n);
  if (!d_codes || !d_offsets || !d_cluster_ptr || !d_cons || !d_cons_len || !d_center || !d_work) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (n > 0x7fffffffLL) return fail(DA_ERR_UNSUPPORTED, "more than 2^31 - 1 pooled sequences");
  int rc;
  if ((rc = cons_table_check(cluster_ptr, n, clusters)) != DA_OK) return rc;
  if (max_len < 0) return fail(DA_ERR_BAD_ARG, "negative max_len");
  if (max_len > 1024) return fail(DA_ERR_UNSUPPORTED, "the alignment kernel takes sequences up to 1024 residues (max_len = %lld)", (long long)max_len);
  if (ld_cons < max_len) return fail(DA_ERR_BAD_ARG, "ld_cons = %lld is smaller than the longest member, %lld", (long long)ld_cons, (long long)max_len);
  if (!matrix_table_host(matrix_id)) return fail(DA_ERR_BAD_ARG, "matrix id %d out of range", matrix_id);
  if ((rc = require_device()) != DA_OK) return rc;
  return launch_cluster_consensus(d_codes, d_offsets, n, cluster_ptr, d_cluster_ptr, clusters, max_len, matrix_id, gap_open, gap_ext, d_cons, ld_cons,
                                  d_cons_len, d_center, d_work, work_bytes, static_cast<hipStream_t>(stream));
}

int da_dev_consensus_center_sums(const int32_t *d_len, const int32_t *d_matches, int64_t pair_begin, int64_t pairs, const int64_t *cluster_ptr,
                                 const int64_t *d_cluster_ptr, int64_t clusters, int64_t *d_pair_ptr, uint64_t *d_sums, void *stream) {
  if (pairs < 0 || pair_begin < 0 || clusters <= 0) return fail(DA_ERR_BAD_ARG, "negative count or no clusters");
  if (!d_len || !d_matches || !d_cluster_ptr || !d_pair_ptr || !d_sums) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  int rc;
  if ((rc = cons_table_check(cluster_ptr, cluster_ptr ? cluster_ptr[clusters] : 0, clusters)) != DA_OK) return rc;
  std::vector<int64_t> pp((size_t)clusters + 1, 0);
  for (int64_t k = 0; k < clusters; ++k) {
    const int64_t c = cluster_ptr[k + 1] - cluster_ptr[k];
    pp[(size_t)k + 1] = pp[(size_t)k] + c * (c - 1);
  }
  if (pair_begin + pairs > pp[(size_t)clusters])
    return fail(DA_ERR_BAD_ARG, "pairs [%lld, %lld) reach past the table's %lld", (long long)pair_begin, (long long)(pair_begin + pairs),
                (long long)pp[(size_t)clusters]);
  if ((rc = require_device()) != DA_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((rc = launch_cons_pair_ptr(d_cluster_ptr, clusters, d_pair_ptr, s)) != DA_OK) return rc;
  return launch_cons_center_sums(d_len, d_matches, pair_begin, pair_begin + pairs, cluster_ptr, pp.data(), d_cluster_ptr, d_pair_ptr, clusters, d_sums, s);
}

int da_dev_consensus_pick(const uint64_t *d_sums, const int64_t *d_cluster_ptr, int64_t clusters, int32_t *d_center, void *stream) {
  if (clusters < 0) return fail(DA_ERR_BAD_ARG, "negative count");
  if (clusters == 0) return DA_OK;
  if (!d_sums || !d_cluster_ptr || !d_center) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  int rc;
  if ((rc = require_device()) != DA_OK) return rc;
  return launch_cons_pick(d_sums, d_cluster_ptr, clusters, d_center, static_cast<hipStream_t>(stream));
}

int da_dev_consensus_vote(const uint8_t *d_codes, const int64_t *d_offsets, const int64_t *d_cluster_ptr, const int32_t *d_center, int64_t cluster_begin,
                          int64_t cluster_count, const uint8_t *d_ops, int64_t ld_ops, const int32_t *d_len, int64_t row_begin, int64_t rows,
                          uint32_t *d_carry, uint8_t *d_cons, int64_t ld_cons, int32_t *d_cons_len, int64_t max_len, void *stream) {
  if (cluster_begin < 0 || cluster_count < 0 || row_begin < 0 || rows < 0 || ld_ops < 0 || ld_cons < 0 || max_len < 0)
    return fail(DA_ERR_BAD_ARG, "negative count");
  if (cluster_count == 0) return DA_OK;
  if (!d_codes || !d_offsets || !d_cluster_ptr || !d_center || !d_carry || !d_cons || !d_cons_len || (rows > 0 && !d_ops))
    return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (max_len > 1024) return fail(DA_ERR_UNSUPPORTED, "centers have up to 1024 residues (max_len = %lld)", (long long)max_len);
  if (ld_cons < max_len) return fail(DA_ERR_BAD_ARG, "ld_cons = %lld is smaller than the longest member, %lld", (long long)ld_cons, (long long)max_len);
  int rc;
  if ((rc = require_device()) != DA_OK) return rc;
  return launch_cons_vote(d_codes, d_offsets, d_cluster_ptr, d_center, cluster_begin, cluster_count, d_ops, ld_ops, d_len, row_begin, row_begin + rows,
                          d_carry, d_cons, ld_cons, d_cons_len, max_len, static_cast<hipStream_t>(stream));
}

int da_cluster_consensus(const uint8_t *residues, const int64_t *offsets, int64_t n, const int32_t *cluster_of, int64_t clusters, const char *matrix_name,
                         int gap_open, int gap_ext, uint8_t *cons_out, int64_t ld_cons, int32_t *cons_len_out, int32_t *center_out) {
  const int mid = da_matrix_id(matrix_name);               // before anything else, as in da_nw_align_long_pairs
  if (mid < 0) return DA_ERR_BAD_MATRIX;
  if (n < 0 || clusters < 0) return fail(DA_ERR_BAD_ARG, "negative count");
  if (n == 0 && clusters == 0) return DA_OK;               // nothing to write
  if (n > 0x7fffffffLL) return fail(DA_ERR_UNSUPPORTED, "more than 2^31 - 1 sequences");
  if (!residues || !cluster_of || !cons_out || !cons_len_out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  int64_t total = 0, longest = 0;
  int rc;
  if ((rc = check_offsets(offsets, n, &total, &longest)) != DA_OK) return rc;
  std::vector<int64_t> size((size_t)clusters, 0);
  for (int64_t i = 0; i < n; ++i) {
    if (cluster_of[i] < 0 || cluster_of[i] >= clusters)
      return fail(DA_ERR_BAD_ARG, "sequence %lld: cluster %d is outside [0, %lld)", (long long)i, (int)cluster_of[i], (long long)clusters);
    ++size[(size_t)cluster_of[i]];
  }
  for (int64_t k = 0; k < clusters; ++k)
    if (size[(size_t)k] == 0) return fail(DA_ERR_BAD_ARG, "cluster %lld has no member", (long long)k);
  // the pool: the members of every cluster of two or more, clusters ascending, members in input order -- what both alignment calls index
  std::vector<int64_t> pool_k, cptr(1, 0), slot((size_t)clusters, -1);
  for (int64_t k = 0; k < clusters; ++k)
    if (size[(size_t)k] > 1) { slot[(size_t)k] = (int64_t)pool_k.size(); pool_k.push_back(k); cptr.push_back(cptr.back() + size[(size_t)k]); }
  const int64_t pk = (int64_t)pool_k.size(), pn = cptr.back();
  std::vector<int32_t> member((size_t)pn), single((size_t)clusters, -1);
  {
    std::vector<int64_t> fill(cptr.begin(), cptr.end() - 1);
    for (int64_t i = 0; i < n; ++i) {
      const int64_t s = slot[(size_t)cluster_of[i]];
      if (s >= 0) member[(size_t)fill[(size_t)s]++] = (int32_t)i; else single[(size_t)cluster_of[i]] = (int32_t)i;
    }
  }
  auto len_of = [&](int64_t g) { return offsets[member[(size_t)g] + 1] - offsets[member[(size_t)g]]; };
  // the length refusal, worded as the first alignment call words it: pairs in its order, i ascending then j != i ascending.  The first pair of a
  // cluster with a long member is (0, 1) if member 0 is long, else (0, the first long member).
  int64_t pair_base = 0, pool_longest = 0;
  for (int64_t s = 0; s < pk; ++s) {
    const int64_t b = cptr[(size_t)s], c = cptr[(size_t)s + 1] - b;
    for (int64_t t = 0; t < c; ++t) {
      if (len_of(b + t) <= 1024) { pool_longest = std::max(pool_longest, len_of(b + t)); continue; }
      const int64_t j = t == 0 ? 1 : t;
      return fail(DA_ERR_UNSUPPORTED, "the alignment kernel takes sequences up to %d residues (pair %lld: %lld and %lld)", 1024,
                  (long long)(pair_base + j - 1), (long long)len_of(b), (long long)len_of(b + j));
    }
    pair_base += c * (c - 1);
  }
  if (ld_cons < longest) return fail(DA_ERR_BAD_ARG, "ld_cons = %lld is smaller than the longest member, %lld", (long long)ld_cons, (long long)longest);
  // the residue error of the first alignment call, from every member's first bad position: member i (not empty) meets, in this order, its own
  // residue 0, the first bad residue of its first partner, its own first bad residue, then the first bad residue of any other member
  {
    const std::vector<int32_t> bad = nw_first_bad(residues, offsets, n);
    auto bad_of = [&](int64_t g) { return bad[(size_t)member[(size_t)g]]; };
    auto chr = [&](int64_t g) { return (char)residues[offsets[member[(size_t)g]] + bad_of(g)]; };
    for (int64_t s = 0; s < pk; ++s) {
      const int64_t b = cptr[(size_t)s], c = cptr[(size_t)s + 1] - b;
      int64_t b1 = -1, b2 = -1;                             // the first two members with a bad residue
      for (int64_t t = 0; t < c && b2 < 0; ++t)
        if (bad_of(b + t) >= 0) { if (b1 < 0) b1 = t; else b2 = t; }
      if (b1 < 0) continue;
      for (int64_t i = 0; i < c; ++i) {
        if (len_of(b + i) == 0) continue;                   // no row runs
        if (bad_of(b + i) == 0) return fail(DA_ERR_BAD_RESIDUE_SEQ1, "Invalid amino acid in sequence1: %c", chr(b + i));
        const int64_t j0 = i == 0 ? 1 : 0;
        if (bad_of(b + j0) >= 0) return fail(DA_ERR_BAD_RESIDUE_SEQ2, "Invalid amino acid in sequence2: %c", chr(b + j0));
        if (bad_of(b + i) > 0) return fail(DA_ERR_BAD_RESIDUE_SEQ1, "Invalid amino acid in sequence1: %c", chr(b + i));
        const int64_t other = b1 != i ? b1 : b2;
        if (other >= 0) return fail(DA_ERR_BAD_RESIDUE_SEQ2, "Invalid amino acid in sequence2: %c", chr(b + other));
      }
    }
  }
  if (pk > 0 && (rc = require_device()) != DA_OK) return rc;   // nothing is written without one
  // a cluster of one is its member, copied through
  for (int64_t k = 0; k < clusters; ++k) {
    if (single[(size_t)k] < 0) continue;
    const int64_t i = single[(size_t)k], ln = offsets[i + 1] - offsets[i];
    memset(cons_out + (size_t)k * (size_t)ld_cons, 0, (size_t)ld_cons);
    memcpy(cons_out + (size_t)k * (size_t)ld_cons, residues + offsets[i], (size_t)ln);
    cons_len_out[k] = (int32_t)ln;
    if (center_out) center_out[k] = (int32_t)i;
  }
  if (pk == 0) return DA_OK;                                // no device needed
  std::vector<int64_t> poff((size_t)pn + 1, 0);
  for (int64_t g = 0; g < pn; ++g) poff[(size_t)g + 1] = poff[(size_t)g] + len_of(g);
  std::vector<uint8_t> pres((size_t)std::max<int64_t>(poff[(size_t)pn], 1));
  for (int64_t g = 0; g < pn; ++g) memcpy(pres.data() + poff[(size_t)g], residues + offsets[member[(size_t)g]], (size_t)len_of(g));
  NwCodes pool;
  if ((rc = pool.upload(pres.data(), poff.data(), pn, poff[(size_t)pn])) != DA_OK) return rc;
  const int64_t ldc = std::max<int64_t>(pool_longest, 1);
  DevBuf dptr, dcons, dlen, dcen, work;
  if ((rc = dptr.alloc((size_t)(pk + 1) * sizeof(int64_t))) != DA_OK || (rc = dcons.alloc((size_t)pk * (size_t)ldc)) != DA_OK ||
      (rc = dlen.alloc((size_t)pk * sizeof(int32_t))) != DA_OK || (rc = dcen.alloc((size_t)pk * sizeof(int32_t))) != DA_OK) return rc;
  DA_HIP_TRY(hipMemcpy(dptr.p, cptr.data(), (size_t)(pk + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  // blocks within DYNAALIGN_BLOCK_BYTES (half of the free memory without it), never less than blocks of 64 pairs take
  const size_t wbytes = std::max(std::min(cluster_consensus_workspace_bytes(cptr.data(), pk, pool_longest, false), block_budget()),
                                 cluster_consensus_workspace_bytes(cptr.data(), pk, pool_longest, true));
  if ((rc = work.alloc(wbytes)) != DA_OK) return rc;
  if ((rc = launch_cluster_consensus(pool.codes.as<uint8_t>(), pool.in.off.as<int64_t>(), pn, cptr.data(), dptr.as<int64_t>(), pk, pool_longest, mid,
                                     gap_open, gap_ext, dcons.as<uint8_t>(), ldc, dlen.as<int32_t>(), dcen.as<int32_t>(), work.p, wbytes, nullptr)) != DA_OK)
    return rc;
  std::vector<uint8_t> hcons((size_t)pk * (size_t)ldc);
  std::vector<int32_t> hlen((size_t)pk), hcen((size_t)pk);
  DA_HIP_TRY(hipMemcpy(hcons.data(), dcons.p, hcons.size(), hipMemcpyDeviceToHost));
  DA_HIP_TRY(hipMemcpy(hlen.data(), dlen.p, (size_t)pk * sizeof(int32_t), hipMemcpyDeviceToHost));
  DA_HIP_TRY(hipMemcpy(hcen.data(), dcen.p, (size_t)pk * sizeof(int32_t), hipMemcpyDeviceToHost));
  if ((rc = sync_or_fail("the consensus kernels failed")) != DA_OK) return rc;
  for (int64_t s = 0; s < pk; ++s) {
    const int64_t k = pool_k[(size_t)s];
    memset(cons_out + (size_t)k * (size_t)ld_cons, 0, (size_t)ld_cons);
    memcpy(cons_out + (size_t)k * (size_t)ld_cons, hcons.data() + (size_t)s * (size_t)ldc, (size_t)hlen[(size_t)s]);
    cons_len_out[k] = hlen[(size_t)s];
    if (center_out) center_out[k] = member[(size_t)hcen[(size_t)s]];
  }
  return DA_OK;
}


// ---- two sets, threshold form: the entries of the rectangle that pass a threshold as a sorted edge list (rect_edges_kernels.hip) ---------
static int rect_block_check(const void *a, const void *b, const void *c, int64_t rows, int64_t n, int64_t ld, int nbins) {
  if (rows < 0 || n < 0) return fail(DA_ERR_BAD_ARG, "negative shape");
  if (!a || !b || !c) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (ld < n) return fail(DA_ERR_BAD_ARG, "ld (%lld) < n (%lld)", (long long)ld, (long long)n);
  if (nbins < 1 || nbins > 65536) return fail(DA_ERR_BAD_ARG, "nbins must be in 1 .. 65536 (got %d)", nbins);
  return DA_OK;
}
int da_dev_rect_histogram(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, int nbins, uint64_t *d_hist, void *stream) {
  int rc;
  if ((rc = rect_block_check(d_keys, d_hist, d_hist, rows, n, ld, nbins)) != DA_OK) return rc;
  return launch_rect_histogram(d_keys, rows, n, ld, nbins, reinterpret_cast<unsigned long long *>(d_hist), static_cast<hipStream_t>(stream));
}
size_t da_dev_threshold_rows_workspace_bytes(int64_t rows) { return threshold_rows_workspace_bytes(rows); }
int da_dev_threshold_rows_count(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, const uint8_t *d_keep, int nbins, int64_t *d_rowptr,
                                void *d_work, size_t work_bytes, void *stream) {
  int rc;
  if ((rc = rect_block_check(d_keys, d_keep, d_rowptr, rows, n, ld, nbins)) != DA_OK) return rc;
  if (!d_work) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  return launch_threshold_rows_count(d_keys, rows, n, ld, d_keep, nbins, d_rowptr, d_work, work_bytes, static_cast<hipStream_t>(stream));
}
int da_dev_threshold_rows_emit(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, const uint8_t *d_keep, int nbins, const int64_t *d_rowptr,
                               int32_t *d_j, uint16_t *d_key_out, int64_t capacity, void *stream) {
  int rc;
  if ((rc = rect_block_check(d_keys, d_keep, d_rowptr, rows, n, ld, nbins)) != DA_OK) return rc;
  if (capacity < 0) return fail(DA_ERR_BAD_ARG, "negative capacity");
  if (capacity > 0 && (!d_j || !d_key_out)) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  return launch_threshold_rows_emit(d_keys, rows, n, ld, d_keep, nbins, d_rowptr, d_j, d_key_out, capacity, static_cast<hipStream_t>(stream));
}

// the threshold argument of the *_cross_edges entry points: a quantile level in [0, 1], or any non-NaN absolute threshold
static int thresh_arg_check(double thresh, int thresh_is_quantile) {
  if (thresh_is_quantile) {
    if (!(thresh >= 0.0 && thresh <= 1.0)) return fail(DA_ERR_BAD_ARG, "thresh_p must be in [0, 1]");
  } else if (thresh != thresh) {
    return fail(DA_ERR_BAD_ARG, "the threshold must not be NaN");
  }
  return DA_OK;
}

// ---- the two-pass threshold driver, written once for uint16 codes with a keep table (CodeKeys) and uint32 value ranks (RankKeys) ----------
}  // extern "C"  (reopened below)
namespace {
// Rows [0, m) of a problem thresholded block by block.  `keys` owns the scratch block of keys.blk rows and knows its key type: produce(b0, b1)
// fills it with the keys of rows [b0, b1) (columns from c0(b0) on), histogram() adds the block to the device histogram of bins() bins,
// quantile() turns the histogram into the threshold, set_threshold() into the keep decision, count() / emit() are the two steps of the
// ordered compaction.  Quantile form: a first pass of produce + histogram over all blocks gives the threshold; a single block is then kept,
// several are produced again.  Per block, in order: the per-row counts and their scan, the 8-byte total read back, then
// sink(b0, b1, d_rowptr_block, total, base) -- base = the kept entries of the blocks before -- emits where it wants them.  Works on, and
// synchronises, keys.stream.
typedef std::function<int(int64_t, int64_t, const int64_t *, int64_t, int64_t)> BlockSink;
template <typename Keys>
int threshold_blocks(Keys &keys, int64_t m, double thresh, bool is_quantile, const BlockSink &sink, double *threshold_out, int64_t *n_edges_out) {
  const hipStream_t stream = keys.stream;
  const int64_t blk = keys.blk, nbins = keys.bins();
  const size_t wb = threshold_rows_workspace_bytes(blk);
  DevBuf rowptr, work, hist;
  int rc;
  if ((rc = rowptr.alloc((size_t)(blk + 1) * 8)) != DA_OK || (rc = work.alloc(wb)) != DA_OK) return rc;
  double thr = thresh;
  bool have_block = false;
  if (is_quantile) {
    if ((rc = hist.alloc((size_t)nbins * 8)) != DA_OK) return rc;
    DA_HIP_TRY(hipMemsetAsync(hist.p, 0, (size_t)nbins * 8, stream));
    for (int64_t b0 = 0; b0 < m; b0 += blk) {
      const int64_t b1 = std::min(m, b0 + blk);
      if ((rc = keys.produce(b0, b1)) != DA_OK || (rc = keys.histogram(b0, b1, hist.as<unsigned long long>())) != DA_OK) return rc;
    }
    std::vector<uint64_t> h((size_t)nbins);
    DA_HIP_TRY(hipMemcpyAsync(h.data(), hist.p, (size_t)nbins * 8, hipMemcpyDeviceToHost, stream));
    DA_HIP_TRY(hipStreamSynchronize(stream));
    hist.release();
    if ((rc = keys.quantile(h, thresh, &thr)) != DA_OK) return rc;
    have_block = blk >= m;
  }
  if ((rc = keys.set_threshold(thr)) != DA_OK) return rc;
  int64_t base = 0;
  for (int64_t b0 = 0; b0 < m; b0 += blk) {
    const int64_t b1 = std::min(m, b0 + blk), rows = b1 - b0;
    if (!have_block && (rc = keys.produce(b0, b1)) != DA_OK) return rc;
    if ((rc = keys.count(b0, b1, rowptr.as<int64_t>(), work.p, wb)) != DA_OK) return rc;
    int64_t total = 0;
    DA_HIP_TRY(hipMemcpyAsync(&total, rowptr.as<int64_t>() + rows, 8, hipMemcpyDeviceToHost, stream));
    DA_HIP_TRY(hipStreamSynchronize(stream));
    if ((rc = sink(b0, b1, rowptr.as<int64_t>(), total, base)) != DA_OK) return rc;
    base += total;
  }
  DA_HIP_TRY(hipStreamSynchronize(stream));
  *threshold_out = thr;
  *n_edges_out = base;
  return DA_OK;
}

// a block's emitted entries appended to the handle's host vectors: i = block origin + row, j = the emit's block-local column + c0,
// w = values[key] (the table the dense calls widen with)
template <typename Key>
int block_to_host(EdgeSet &es, const std::vector<double> &values, int64_t b0, int64_t rows, int64_t c0, const int64_t *d_rowptr, const int32_t *d_j,
                  const Key *d_key, int64_t total, int64_t base, hipStream_t stream) {
  const size_t at = (size_t)base, end = (size_t)(base + total);
  es.i.resize(end); es.j.resize(end); es.w.resize(end);
  std::vector<int64_t> rp((size_t)rows + 1);
  std::vector<Key> key((size_t)total);
  DA_HIP_TRY(hipMemcpyAsync(rp.data(), d_rowptr, (size_t)(rows + 1) * 8, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipMemcpyAsync(es.j.data() + at, d_j, (size_t)total * 4, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipMemcpyAsync(key.data(), d_key, (size_t)total * sizeof(Key), hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipStreamSynchronize(stream));
  for (int64_t r = 0; r < rows; ++r)
    for (int64_t e = rp[(size_t)r]; e < rp[(size_t)r + 1]; ++e) es.i[at + (size_t)e] = (int32_t)(b0 + r);
  for (int64_t e = 0; e < total; ++e) {
    es.j[at + (size_t)e] += (int32_t)c0;
    es.w[at + (size_t)e] = values[key[(size_t)e]];
  }
  return DA_OK;
}
// the host route: the keys' scratch block, then the driver with a sink that emits each block and appends it to the handle
template <typename Keys>
int edges_to_host(Keys &keys, int64_t m, double thresh, bool is_quantile, EdgeSet &es, int64_t *n_edges) {
  typedef typename Keys::Key Key;
  int rc;
  if ((rc = keys.init()) != DA_OK) return rc;
  return threshold_blocks(keys, m, thresh, is_quantile, [&](int64_t b0, int64_t b1, const int64_t *d_rowptr, int64_t total, int64_t base) -> int {
    if (total <= 0) return DA_OK;
    DevBuf dj, dkey;
    int rc2;
    if ((rc2 = dj.alloc((size_t)total * 4)) != DA_OK || (rc2 = dkey.alloc((size_t)total * sizeof(Key))) != DA_OK ||
        (rc2 = keys.emit(b0, b1, d_rowptr, dj.as<int32_t>(), dkey.as<Key>(), total)) != DA_OK) return rc2;
    return block_to_host<Key>(es, keys.values, b0, b1 - b0, keys.c0(b0), d_rowptr, dj.as<int32_t>(), dkey.as<Key>(), total, base, keys.stream);
  }, &es.threshold, n_edges);
}

// uint16 counts / codes of an m x n rectangle (blocks as topk_blocks: compute(b0, b1, d, ld) writes the codes of rows [b0, b1) to the scratch
// block d).  values[code] is the similarity a code stands for; a code is kept when its value is positive and not below the threshold.
typedef std::function<int(int64_t, int64_t, void *, int64_t)> RectCompute;
struct CodeKeys {
  typedef uint16_t Key;
  const std::vector<double> &values;
  const RectCompute compute;
  const hipStream_t stream;
  const int64_t n, ld, blk;
  DevBuf d, keep;
  std::vector<uint8_t> kp;                    // the host image of keep[]: alive until the copy has run
  CodeKeys(int64_t m, int64_t n_, const std::vector<double> &values_, const RectCompute &compute_, hipStream_t stream_)
      : values(values_), compute(compute_), stream(stream_), n(n_), ld((n_ + 7) / 8 * 8), blk(std::min(block_rows(ld, sizeof(uint16_t)), m)) {}
  int init() {
    int rc;
    if ((rc = d.alloc((size_t)blk * (size_t)ld * sizeof(uint16_t))) != DA_OK) return rc;
    return keep.alloc(values.size());
  }
  int64_t bins() const { return (int64_t)values.size(); }
  int64_t c0(int64_t) const { return 0; }
  int produce(int64_t b0, int64_t b1) { return compute(b0, b1, d.p, ld); }
  int histogram(int64_t b0, int64_t b1, unsigned long long *d_hist) {
    return launch_rect_histogram(d.as<uint16_t>(), b1 - b0, n, ld, (int)bins(), d_hist, stream);
  }
  int quantile(const std::vector<uint64_t> &h, double p, double *thr) const {
    // order statistics need the codes in ascending order of their VALUE (MH: already so; NW: ratios, equal values side by side)
    const int nbins = (int)bins();
    std::vector<int> order((size_t)nbins);
    for (int b = 0; b < nbins; ++b) order[(size_t)b] = b;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return values[(size_t)a] < values[(size_t)b]; });
    std::vector<uint64_t> hs((size_t)nbins);
    std::vector<double> vs((size_t)nbins);
    for (int b = 0; b < nbins; ++b) { hs[(size_t)b] = h[(size_t)order[(size_t)b]]; vs[(size_t)b] = values[(size_t)order[(size_t)b]]; }
    return da_quantile_type7(hs.data(), vs.data(), nbins, p, thr);
  }
  int set_threshold(double thr) {
    kp.resize(values.size());
    for (size_t b = 0; b < kp.size(); ++b) kp[b] = (values[b] > 0.0 && values[b] >= thr) ? 1 : 0;
    DA_HIP_TRY(hipMemcpyAsync(keep.p, kp.data(), kp.size(), hipMemcpyHostToDevice, stream));
    return DA_OK;
  }
  int count(int64_t b0, int64_t b1, int64_t *d_rowptr, void *d_work, size_t work_bytes) {
    return launch_threshold_rows_count(d.as<uint16_t>(), b1 - b0, n, ld, keep.as<uint8_t>(), (int)bins(), d_rowptr, d_work, work_bytes, stream);
  }
  int emit(int64_t b0, int64_t b1, const int64_t *d_rowptr, int32_t *d_j, uint16_t *d_key, int64_t capacity) {
    return launch_threshold_rows_emit(d.as<uint16_t>(), b1 - b0, n, ld, keep.as<uint8_t>(), (int)bins(), d_rowptr, d_j, d_key, capacity, stream);
  }
};
}  // namespace
extern "C" {

int da_similarity_mh_cross_edges_begin(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues,
                                       const int64_t *y_offsets, int64_t n, int k, int n_hash, const uint32_t *seeds, double thresh,
                                       int thresh_is_quantile, da_edges **handle_out, double *threshold_out, int64_t *n_edges_out) {
  return edges_run_handle(handle_out, threshold_out, n_edges_out, [&](bool, EdgeSet &es, int64_t *n_edges) -> int {
    int rc;
    int64_t x_total, y_total;
    if ((rc = mh_cross_host_validate(x_residues, x_offsets, m, y_residues, y_offsets, n, k, n_hash, seeds, &rc, &x_total, &y_total)) != DA_OK) return rc;
    if ((rc = thresh_arg_check(thresh, thresh_is_quantile)) != DA_OK) return rc;
    if ((rc = require_device()) != DA_OK) return rc;
    DeviceInput dx, dy;
    if ((rc = dx.upload(x_residues, x_offsets, m, x_total, seeds, n_hash)) != DA_OK || (rc = dy.upload(y_residues, y_offsets, n, y_total, nullptr, 0)) != DA_OK)
      return rc;
    MhCrossOperand c;
    if ((rc = mh_cross_operand(dx.res.as<uint8_t>(), dx.off.as<int64_t>(), m, dy.res.as<uint8_t>(), dy.off.as<int64_t>(), n, k, n_hash,
                               dx.seeds.as<uint32_t>(), &c, nullptr)) != DA_OK) return rc;
    DA_HIP_TRY(hipStreamSynchronize(nullptr));
    c.work.release(); c.sig.release();                     // before the scratch block is sized
    const std::vector<double> values = mh_code_values(n_hash);
    CodeKeys keys(m, n, values, [&](int64_t b0, int64_t b1, void *d, int64_t ld) { return mh_cross_compare(c, n_hash, b0, b1, DA_OUT_COMPACT, d, ld, nullptr); },
                  nullptr);
    return edges_to_host(keys, m, thresh, thresh_is_quantile != 0, es, n_edges);
  });
}

int da_similarity_nw_cross_edges_begin(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues,
                                       const int64_t *y_offsets, int64_t n, const char *matrix_name, int gap_open, int gap_ext, double thresh,
                                       int thresh_is_quantile, da_edges **handle_out, double *threshold_out, int64_t *n_edges_out) {
  return edges_run_handle(handle_out, threshold_out, n_edges_out, [&](bool, EdgeSet &es, int64_t *n_edges) -> int {
    const int mid = da_matrix_id(matrix_name);             // before anything else, as in similarityNW
    if (mid < 0) return DA_ERR_BAD_MATRIX;
    int rc;
    if (m <= 0 || n <= 0) {                                // an empty rectangle: no edges; it has no quantile
      if ((rc = thresh_arg_check(thresh, thresh_is_quantile)) != DA_OK) return rc;
      if (thresh_is_quantile) return fail(DA_ERR_BAD_ARG, "quantile of an empty set");
      es.threshold = thresh;
      *n_edges = 0;
      return DA_OK;
    }
    NwCross c{x_residues, y_residues, x_offsets, y_offsets, m, n, mid, gap_open, gap_ext};
    if ((rc = c.check(true, [&] { return thresh_arg_check(thresh, thresh_is_quantile); }, "a quantile", 127,
                      "the NW two-set edge list works on uint16 codes: sequences up to 127 residues")) != DA_OK || (rc = c.upload()) != DA_OK) return rc;
    const int64_t max_len = c.max_len;
    // every code that can occur lies below this bound (matches <= max_len, length <= 2 * max_len), as in the square NW edge path: the
    // histogram of short peptides stays in LDS; length 0 cannot occur (no empty sequences)
    const int nbins = (int)((max_len << 8) | (2 * max_len)) + 1;
    const std::vector<double> values = nw_code_values(nbins, 0.0);
    CodeKeys keys(m, n, values, [&](int64_t b0, int64_t b1, void *d, int64_t ld) { return c.rows(b0, b1, DA_OUT_COMPACT, d, ld, nullptr); }, nullptr);
    return edges_to_host(keys, m, thresh, thresh_is_quantile != 0, es, n_edges);
  });
}

int da_dev_similarity_mh_cross_edges(const uint8_t *d_x_residues, const int64_t *d_x_offsets, int64_t m, const uint8_t *d_y_residues,
                                     const int64_t *d_y_offsets, int64_t n, int k, int n_hash, const uint32_t *d_seeds, double thresh,
                                     int thresh_is_quantile, int64_t *d_rowptr, int32_t *d_j, double *d_w, int64_t capacity, double *threshold_out,
                                     int64_t *n_edges_out, void *stream_v) {
  int rc;
  if ((rc = validate_mh(m, k > 0 ? k : 1, n_hash > 0 ? n_hash : 1)) != DA_OK || (rc = validate_mh(n, k, n_hash)) != DA_OK) return rc;   // x empty, y empty, k, n_hash
  if (!d_x_residues || !d_x_offsets || !d_y_residues || !d_y_offsets || !d_seeds || !d_rowptr || !threshold_out || !n_edges_out)
    return fail(DA_ERR_BAD_ARG, "NULL pointer");
  if (n_hash > 65535) return fail(DA_ERR_UNSUPPORTED, "the compare kernel counts in 16 bits: the two-set calls take n_hash <= 65535 (got %d)", n_hash);
  if (m > 0x7ffffff0LL || n > 0x7ffffff0LL) return fail(DA_ERR_UNSUPPORTED, "two-set MinHash: too many sequences");
  if ((rc = thresh_arg_check(thresh, thresh_is_quantile)) != DA_OK) return rc;
  if (capacity < 0) return fail(DA_ERR_BAD_ARG, "negative capacity");
  if (capacity > 0 && (!d_j || !d_w)) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  MhCrossOperand c;
  if ((rc = mh_cross_operand(d_x_residues, d_x_offsets, m, d_y_residues, d_y_offsets, n, k, n_hash, d_seeds, &c, stream)) != DA_OK) return rc;
  DA_HIP_TRY(hipStreamSynchronize(stream));
  c.work.release(); c.sig.release();                       // before the scratch block is sized
  const std::vector<double> values = mh_code_values(n_hash);
  CodeKeys keys(m, n, values, [&](int64_t b0, int64_t b1, void *d, int64_t ld) { return mh_cross_compare(c, n_hash, b0, b1, DA_OUT_COMPACT, d, ld, stream); },
                stream);
  if ((rc = keys.init()) != DA_OK) return rc;
  // the device-resident sink: the block's row pointers placed into the caller's, its entries emitted straight behind those of the blocks before
  return threshold_blocks(keys, m, thresh, thresh_is_quantile != 0, [&](int64_t b0, int64_t b1, const int64_t *rp, int64_t total, int64_t base) -> int {
                            int rc2;
                            const int64_t rows = b1 - b0;   // the last block also places the total
                            if ((rc2 = launch_rowptr_offset(rp, rows + (b1 == m ? 1 : 0), base, d_rowptr + b0, stream)) != DA_OK) return rc2;
                            const int64_t cnt = std::min(total, capacity - base);
                            if (cnt <= 0) return DA_OK;
                            DevBuf key;
                            if ((rc2 = key.alloc((size_t)cnt * 2)) != DA_OK) return rc2;
                            if ((rc2 = keys.emit(b0, b1, rp, d_j + base, key.as<uint16_t>(), cnt)) != DA_OK ||
                                (rc2 = launch_edge_values(key.as<uint16_t>(), cnt, n_hash, d_w + base, stream)) != DA_OK) return rc2;
                            DA_HIP_TRY(hipStreamSynchronize(stream));   // the key block goes back to the cache after this
                            return DA_OK;
                          }, threshold_out, n_edges_out);
}

// ---- MinHash LSH banding: the one-set entries and the pipelines of both forms (lsh_kernels.hip) ----------------------------------------------
}  // extern "C"  (reopened below)
namespace {
struct LshRoute { int64_t buckets = 0, incidences = 0, verified = 0, edges = 0; };
// Declared AFTER the DevBufs of a scope that launches on a caller's stream: whichever way the scope is left -- an early return after a launch
// included -- the stream is drained before those buffers go back to the cache.
struct StreamDrain {
  hipStream_t stream;
  ~StreamDrain() { (void)hipStreamSynchronize(stream); }
};
LshRoute &lsh_route() { static thread_local LshRoute r; return r; }

// bands, rows, threshold and the cap of the LSH calls, in the order include/dynaalign.h gives
// (top: of the nearest-neighbour calls, checked between the cap and the 16-bit limit; nullptr for the edge calls)
// (edge_text: the 16-bit limit in the edge calls' words although top is given -- the NW lists, which take the edge calls' checks and texts)
int lsh_arg_check(int n_hash, int bands, int rows, double threshold, int64_t max_candidates, const int *top = nullptr, bool edge_text = false) {
  if (bands < 1) return fail(DA_ERR_BAD_ARG, "bands must be >= 1 (got %d)", bands);
  if (rows < 1) return fail(DA_ERR_BAD_ARG, "rows must be >= 1 (got %d)", rows);
  if ((int64_t)bands * rows > n_hash) return fail(DA_ERR_BAD_ARG, "bands * rows = %lld exceeds n_hash = %d", (long long)bands * rows, n_hash);
  if (!(threshold >= 0.0 && threshold <= 1.0)) return fail(DA_ERR_BAD_ARG, "the threshold must be in [0, 1]");
  if (max_candidates < 0) return fail(DA_ERR_BAD_ARG, "max_candidates must be >= 0 (got %lld)", (long long)max_candidates);
  if (top && (*top < 1 || *top > DA_TOPK_MAX)) return fail(DA_ERR_BAD_ARG, "top must be in 1 .. %d (got %d)", DA_TOPK_MAX, *top);
  if (n_hash > 65535)
    return fail(DA_ERR_UNSUPPORTED, "the LSH %s in 16 bits: n_hash <= 65535 (got %d)", top && !edge_text ? "nearest-neighbour lists count" : "edge list counts", n_hash);
  return DA_OK;
}
// the smallest count whose similarity -- the divide of mh_code_values -- reaches the threshold (n_hash + 1: none does)
uint32_t lsh_c_min(int n_hash, double threshold) {
  const std::vector<double> values = mh_code_values(n_hash);
  uint32_t c = 0;
  while (c <= (uint32_t)n_hash && !(values[c] >= threshold)) ++c;
  return c;
}
int lsh_elements_check(const char *what, int64_t n, int bands) {
  if (n > 0x7ffffff0LL || n * (int64_t)bands > LSH_MAX_ELEMENTS)
    return fail(DA_ERR_UNSUPPORTED, "lsh: %s * bands = %lld (sequence, band) elements, at most %lld in one call", what, (long long)(n * (int64_t)bands),
                (long long)LSH_MAX_ELEMENTS);
  return DA_OK;
}
int lsh_index_mismatch(int64_t n, int bands, int rows) {
  return fail(DA_ERR_BAD_ARG, "lsh: the index was not built for n = %lld, bands = %d, rows = %d", (long long)n, bands, rows);
}
// What a pipeline runs on: the m rows of x against the n rows of y through y's built index, or -- d_index NULL -- one set against itself:
// y is x, and the buckets are made inside the workspace.
struct LshSets {
  const void *d_index;
  const uint32_t *x;
  int64_t m, ld_x;
  const uint32_t *y;
  int64_t n, ld_y;
  int n_hash, bands, rows;
};
LshSets lsh_one_set(const uint32_t *d_sig, int64_t n, int64_t ld_sig, int n_hash, int bands, int rows) {
  return LshSets{nullptr, d_sig, n, ld_sig, d_sig, n, ld_sig, n_hash, bands, rows};
}
// What the edge list and the lists share: a front end's slots (they point into the caller's workspace or the index), the verdict of every
// incidence slot (cnt, keep), the kept slots per chunk of 64 and their exclusive sum (coff); `kept` and `firsts` (the distinct candidate
// pairs) are read back, so the stream is synchronised.
struct LshVerdicts {
  DevBuf cnt, keep, ckept, coff, distinct, temp;
  LshSlots slots{};
  int64_t inc = 0, kept = 0;
  uint64_t firsts = 0;
};
// behind either front end: the route's counts, the cap, the verdicts
int lsh_verify_slots(const LshSets &s, uint32_t buckets, uint32_t largest, double threshold, int64_t max_candidates, LshVerdicts &v, hipStream_t stream) {
  int rc;
  LshRoute &route = lsh_route();
  route = LshRoute();
  route.buckets = buckets;
  route.incidences = v.inc;
  if (v.inc > max_candidates)
    return fail(DA_ERR_UNSUPPORTED, "lsh: %lld (pair, band) candidates exceed max_candidates = %lld (largest bucket: %u sequences); use more rows per band",
                (long long)v.inc, (long long)max_candidates, largest);
  const int64_t chunks = ceil_div(v.inc, 64);
  if (chunks + 1 > 0x7ffffff0LL) return fail(DA_ERR_UNSUPPORTED, "lsh: %lld candidates are more than one call verifies", (long long)v.inc);
  const size_t scan_b = lsh_chunk_scan_bytes(v.inc);
  if ((rc = v.cnt.alloc((size_t)v.inc * 2)) != DA_OK || (rc = v.keep.alloc((size_t)v.inc)) != DA_OK || (rc = v.ckept.alloc((size_t)(chunks + 1) * 8)) != DA_OK ||
      (rc = v.coff.alloc((size_t)(chunks + 1) * 8)) != DA_OK || (rc = v.distinct.alloc(8)) != DA_OK || (rc = v.temp.alloc(scan_b)) != DA_OK) return rc;
  if ((rc = launch_lsh_verify_enumerated(s.x, s.m, s.ld_x, s.y, s.n, s.ld_y, s.n_hash, s.rows, lsh_c_min(s.n_hash, threshold), v.slots, v.inc,
                                         v.cnt.as<uint16_t>(), v.keep.as<uint8_t>(), v.ckept.as<int64_t>(), v.coff.as<int64_t>(), v.distinct.as<uint64_t>(),
                                         v.temp.p, scan_b, stream)) != DA_OK)
    return rc;
  DA_HIP_TRY(hipMemcpyAsync(&v.kept, v.coff.as<int64_t>() + chunks, 8, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipMemcpyAsync(&v.firsts, v.distinct.p, 8, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipStreamSynchronize(stream));
  v.temp.release();
  return DA_OK;
}
// the two front ends: the buckets of one set; the probe of y's index, refused when the index was built for something else
int lsh_verdicts(const LshSets &s, double threshold, int64_t max_candidates, void *d_work, size_t work_bytes, LshVerdicts &v, hipStream_t stream) {
  int rc;
  uint32_t stats[2] = {0, 0};
  if ((rc = lsh_elements_check("n", s.n, s.bands)) != DA_OK) return rc;
  if ((rc = lsh_buckets(s.x, s.n, s.ld_x, s.bands, s.rows, d_work, work_bytes, &v.slots, stats, &v.inc, stream)) != DA_OK) return rc;
  return lsh_verify_slots(s, stats[1], stats[0], threshold, max_candidates, v, stream);
}
int lsh_cross_verdicts(const LshSets &s, double threshold, int64_t max_candidates, void *d_work, size_t work_bytes, LshVerdicts &v, hipStream_t stream) {
  int rc;
  uint32_t stats[3] = {0, 0, 0};
  if ((rc = lsh_cross_probe(s.d_index, s.n, s.x, s.m, s.ld_x, s.bands, s.rows, d_work, work_bytes, &v.slots, stats, &v.inc, stream)) != DA_OK) return rc;
  if (stats[2]) return lsh_index_mismatch(s.n, s.bands, s.rows);
  return lsh_verify_slots(s, stats[1], stats[0], threshold, max_candidates, v, stream);
}
// The edge pipeline on resident signatures.  The sorted list (edges entries: i << 32 | j, count) is left in key / val.  One set always has
// its n diagonal entries; two sets without a kept pair allocate and launch nothing.
int lsh_edges_device(const LshSets &s, double threshold, int64_t max_candidates, void *d_work, size_t work_bytes, DevBuf &key, DevBuf &val,
                     int64_t *edges_out, hipStream_t stream) {
  int rc;
  LshVerdicts v;
  DevBuf temp, key_in, val_in;
  const StreamDrain drain{stream};
  if ((rc = (s.d_index ? lsh_cross_verdicts : lsh_verdicts)(s, threshold, max_candidates, d_work, work_bytes, v, stream)) != DA_OK) return rc;
  const int64_t diagonal_n = s.d_index ? 0 : s.n;
  const int64_t edges = diagonal_n + v.kept;
  if (edges > 0x7ffffff0LL) return fail(DA_ERR_UNSUPPORTED, "lsh: %lld edges are more than one call sorts", (long long)edges);
  if (edges > 0) {
    const size_t sort_b = lsh_edge_sort_bytes(edges);
    if ((rc = key_in.alloc((size_t)edges * 8)) != DA_OK || (rc = val_in.alloc((size_t)edges * 2)) != DA_OK || (rc = key.alloc((size_t)edges * 8)) != DA_OK ||
        (rc = val.alloc((size_t)edges * 2)) != DA_OK || (rc = temp.alloc(sort_b)) != DA_OK) return rc;
    if ((rc = launch_lsh_emit_sort(v.slots, s.m, diagonal_n, s.n_hash, v.inc, v.cnt.as<uint16_t>(), v.keep.as<uint8_t>(), v.coff.as<int64_t>(), edges,
                                   key_in.as<uint64_t>(), val_in.as<uint16_t>(), key.as<uint64_t>(), val.as<uint16_t>(), temp.p, sort_b, stream)) != DA_OK) return rc;
    DA_HIP_TRY(hipStreamSynchronize(stream));
  }
  LshRoute &route = lsh_route();
  route.verified = (int64_t)v.firsts;
  route.edges = edges;
  *edges_out = edges;
  return DA_OK;
}
int lsh_dev_check(const void *d_sig, int64_t n, int64_t ld_sig, int n_hash, int bands, int rows, double threshold, const int *top = nullptr) {
  if (n < 0) return fail(DA_ERR_BAD_ARG, "negative shape");
  if (n_hash <= 0) return fail(DA_ERR_BAD_NHASH, "%s", da_status_message(DA_ERR_BAD_NHASH));
  if (!d_sig) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (ld_sig < n_hash) return fail(DA_ERR_BAD_ARG, "ld_sig (%lld) < n_hash (%d)", (long long)ld_sig, n_hash);
  return lsh_arg_check(n_hash, bands, rows, threshold, 0, top);
}
// The list pipeline on resident signatures: the verdicts, then the entries -- both directions of every kept pair of one set, the x rows of
// two sets -- and the selection into d_idx / d_key ((m, top), leading dimension top).  Synchronises the stream (totals are read back).
int lsh_lists_device(const LshSets &s, double threshold, int top, int64_t max_candidates, void *d_work, size_t work_bytes, int32_t *d_idx, uint16_t *d_key,
                     hipStream_t stream) {
  int rc;
  LshVerdicts v;
  DevBuf temp, cursor, ptr, col, ecnt, written;
  const StreamDrain drain{stream};
  if ((rc = (s.d_index ? lsh_cross_verdicts : lsh_verdicts)(s, threshold, max_candidates, d_work, work_bytes, v, stream)) != DA_OK) return rc;
  const bool both = !s.d_index;
  const int64_t m = s.m, entries = both ? 2 * v.kept : v.kept;
  const size_t scan_b = lsh_knn_scan_bytes(m);
  if ((rc = cursor.alloc((size_t)(m + 1) * 8)) != DA_OK || (rc = ptr.alloc((size_t)(m + 1) * 8)) != DA_OK || (rc = col.alloc((size_t)entries * 4)) != DA_OK ||
      (rc = ecnt.alloc((size_t)entries * 2)) != DA_OK || (rc = written.alloc(8)) != DA_OK || (rc = temp.alloc(scan_b)) != DA_OK) return rc;
  if ((rc = launch_lsh_knn_entries(v.slots, m, both, v.inc, v.cnt.as<uint16_t>(), v.keep.as<uint8_t>(), entries, top, cursor.as<int64_t>(),
                                   ptr.as<int64_t>(), col.as<int32_t>(), ecnt.as<uint16_t>(), written.as<uint64_t>(), temp.p, scan_b, stream)) != DA_OK ||
      (rc = launch_lsh_knn_select(ptr.as<int64_t>(), entries, col.as<int32_t>(), ecnt.as<uint16_t>(), m, top, d_idx, top, d_key, top, stream)) != DA_OK)
    return rc;
  uint64_t entries_written = 0;
  DA_HIP_TRY(hipMemcpyAsync(&entries_written, written.p, 8, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipStreamSynchronize(stream));
  LshRoute &route = lsh_route();
  route.verified = (int64_t)v.firsts;
  route.edges = (int64_t)entries_written;
  return DA_OK;
}
// The components pipeline on resident signatures (one set): the verdicts, then the union step over the kept slots and the renumbering.
// d_work: lsh_workspace_bytes(n, bands) bytes for the buckets, then components_workspace_bytes(n).  Nothing is emitted or sorted.
int lsh_components_device(const LshSets &s, double threshold, int64_t max_candidates, void *d_work, size_t work_bytes, int32_t *d_membership,
                          int32_t *d_sizes, int64_t *n_components_out, hipStream_t stream) {
  int rc;
  if ((rc = lsh_elements_check("n", s.n, s.bands)) != DA_OK) return rc;
  const size_t lsh_b = lsh_workspace_bytes(s.n, s.bands), cc_b = components_workspace_bytes(s.n);
  if (work_bytes < lsh_b + cc_b) return fail(DA_ERR_BAD_ARG, "lsh: workspace too small (%zu bytes, %zu needed)", work_bytes, lsh_b + cc_b);
  LshVerdicts v;
  const StreamDrain drain{stream};
  if ((rc = lsh_verdicts(s, threshold, max_candidates, d_work, lsh_b, v, stream)) != DA_OK) return rc;
  void *cc_work = static_cast<char *>(d_work) + lsh_b;
  int32_t *parent = nullptr;
  if ((rc = launch_cc_init(s.n, cc_work, cc_b, &parent, stream)) != DA_OK ||
      (rc = launch_lsh_union(v.slots, v.inc, v.keep.as<uint8_t>(), parent, stream)) != DA_OK ||
      (rc = launch_cc_finish(s.n, cc_work, cc_b, d_membership, d_sizes, n_components_out, stream)) != DA_OK) return rc;
  LshRoute &route = lsh_route();
  route.verified = (int64_t)v.firsts;
  route.edges = s.n + v.kept;                               // what the edge form would have emitted
  return DA_OK;
}
}  // namespace
extern "C" {

size_t da_dev_lsh_workspace_bytes(int64_t n, int bands) { return lsh_workspace_bytes(n, bands); }

int da_dev_lsh_band_keys(const uint32_t *d_sig, int64_t n, int64_t ld_sig, int n_hash, int bands, int rows, uint64_t *d_keys, int32_t *d_ids,
                         void *stream) {
  int rc;
  if ((rc = lsh_dev_check(d_sig, n, ld_sig, n_hash, bands, rows, 0.0)) != DA_OK) return rc;
  if (n > 0 && (!d_keys || !d_ids)) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  return launch_lsh_band_keys(d_sig, n, ld_sig, bands, rows, d_keys, d_ids, static_cast<hipStream_t>(stream));
}

int da_dev_lsh_verify_pairs(const uint32_t *d_sig, int64_t n, int64_t ld_sig, int n_hash, int bands, int rows, double threshold, const int32_t *d_i,
                            const int32_t *d_j, const int32_t *d_band, int64_t n_triples, uint16_t *d_count, uint8_t *d_keep, void *stream) {
  int rc;
  if ((rc = lsh_dev_check(d_sig, n, ld_sig, n_hash, bands, rows, threshold)) != DA_OK) return rc;
  if (n_triples < 0) return fail(DA_ERR_BAD_ARG, "negative shape");
  if (n_triples > 0 && (!d_i || !d_j || !d_band || !d_count || !d_keep)) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  return launch_lsh_verify_listed(d_sig, n, ld_sig, d_sig, n, ld_sig, n_hash, bands, rows, lsh_c_min(n_hash, threshold), d_i, d_j, d_band, n_triples, d_count,
                                  d_keep, static_cast<hipStream_t>(stream));
}

int da_dev_lsh_edges(const uint32_t *d_sig, int64_t n, int64_t ld_sig, int n_hash, int bands, int rows, double threshold, int64_t max_candidates,
                     void *d_work, size_t work_bytes, int32_t *d_i, int32_t *d_j, uint16_t *d_count, int64_t capacity, int64_t *n_edges_out,
                     void *stream_v) {
  int rc;
  if (n <= 0) return fail(DA_ERR_EMPTY_INPUT, "%s", da_status_message(DA_ERR_EMPTY_INPUT));
  if ((rc = lsh_dev_check(d_sig, n, ld_sig, n_hash, bands, rows, threshold)) != DA_OK) return rc;
  if (max_candidates < 0) return fail(DA_ERR_BAD_ARG, "max_candidates must be >= 0 (got %lld)", (long long)max_candidates);
  if (!n_edges_out || !d_work) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  if (capacity < 0) return fail(DA_ERR_BAD_ARG, "negative capacity");
  if (capacity > 0 && (!d_i || !d_j || !d_count)) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  DevBuf key, val;
  const StreamDrain drain{stream};
  int64_t edges = 0;
  if ((rc = lsh_edges_device(lsh_one_set(d_sig, n, ld_sig, n_hash, bands, rows), threshold, max_candidates, d_work, work_bytes, key, val, &edges, stream)) != DA_OK) return rc;
  if ((rc = launch_lsh_split(key.as<uint64_t>(), val.as<uint16_t>(), std::min(edges, capacity), d_i, d_j, d_count, stream)) != DA_OK) return rc;
  DA_HIP_TRY(hipStreamSynchronize(stream));
  *n_edges_out = edges;
  return DA_OK;
}

int da_similarity_mh_lsh_edges_begin(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, int n_hash, const uint32_t *seeds, int bands,
                                     int rows, double threshold, int64_t max_candidates, da_edges **handle_out, int64_t *n_edges_out) {
  int rc = validate_mh(n, k, n_hash);
  if (rc != DA_OK) return rc;
  if (!residues || !seeds || !handle_out || !n_edges_out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  *handle_out = nullptr;
  int64_t total, max_len;
  if ((rc = check_offsets(offsets, n, &total, &max_len)) != DA_OK) return rc;
  if ((rc = lsh_arg_check(n_hash, bands, rows, threshold, max_candidates)) != DA_OK) return rc;
  if ((rc = require_device()) != DA_OK) return rc;
  MhPlanes mh;
  DevBuf work, key, val;
  const StreamDrain drain{nullptr};
  if ((rc = mh.in.upload(residues, offsets, n, total, seeds, n_hash)) != DA_OK) return rc;
  if ((rc = mh.alloc(n, n_hash, false)) != DA_OK || (rc = mh.signatures(k, 0, n_hash)) != DA_OK) return rc;
  const size_t wb = lsh_workspace_bytes(n, bands);
  if ((rc = work.alloc(wb)) != DA_OK) return rc;
  int64_t edges = 0;
  if ((rc = lsh_edges_device(lsh_one_set(mh.sig.as<uint32_t>(), n, mh.lds, n_hash, bands, rows), threshold, max_candidates, work.p, wb, key, val, &edges, nullptr)) != DA_OK)
    return rc;
  std::unique_ptr<da_edges> h(new da_edges);
  std::vector<uint64_t> hk((size_t)edges);
  std::vector<uint16_t> hv((size_t)edges);
  DA_HIP_TRY(hipMemcpy(hk.data(), key.p, (size_t)edges * 8, hipMemcpyDeviceToHost));
  DA_HIP_TRY(hipMemcpy(hv.data(), val.p, (size_t)edges * 2, hipMemcpyDeviceToHost));
  const std::vector<double> values = mh_code_values(n_hash);
  EdgeSet &es = h->es;
  es.threshold = threshold;
  es.i.resize((size_t)edges); es.j.resize((size_t)edges); es.w.resize((size_t)edges);
  for (size_t e = 0; e < (size_t)edges; ++e) {
    es.i[e] = (int32_t)(hk[e] >> 32);
    es.j[e] = (int32_t)(hk[e] & 0xFFFFFFFFull);
    es.w[e] = values[hv[e]];
  }
  h->n_edges = edges;
  *n_edges_out = edges;
  *handle_out = h.release();
  return DA_OK;
}

int da_dev_lsh_knn_select(const int64_t *d_ptr, int64_t nnz, const int32_t *d_col, const uint16_t *d_count, int64_t n, int top, int32_t *d_idx,
                          int64_t ld_idx, uint16_t *d_key, int64_t ld_key, void *stream) {
  if (n <= 0) return fail(DA_ERR_EMPTY_INPUT, "%s", da_status_message(DA_ERR_EMPTY_INPUT));
  if (top < 1 || top > DA_TOPK_MAX) return fail(DA_ERR_BAD_ARG, "top must be in 1 .. %d (got %d)", DA_TOPK_MAX, top);
  if (nnz < 0) return fail(DA_ERR_BAD_ARG, "negative shape");
  if (ld_idx < top || ld_key < top) return fail(DA_ERR_BAD_ARG, "ld (%lld) < top (%d)", (long long)std::min(ld_idx, ld_key), top);
  if (!d_ptr || !d_idx || !d_key || (nnz > 0 && (!d_col || !d_count))) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  return launch_lsh_knn_select(d_ptr, nnz, d_col, d_count, n, top, d_idx, ld_idx, d_key, ld_key, static_cast<hipStream_t>(stream));
}

int da_dev_lsh_knn(const uint32_t *d_sig, int64_t n, int64_t ld_sig, int n_hash, int bands, int rows, double threshold, int top, int64_t max_candidates,
                   void *d_work, size_t work_bytes, int32_t *d_idx, uint16_t *d_key, void *stream) {
  int rc;
  if (n <= 0) return fail(DA_ERR_EMPTY_INPUT, "%s", da_status_message(DA_ERR_EMPTY_INPUT));
  if ((rc = lsh_dev_check(d_sig, n, ld_sig, n_hash, bands, rows, threshold, &top)) != DA_OK) return rc;
  if (max_candidates < 0) return fail(DA_ERR_BAD_ARG, "max_candidates must be >= 0 (got %lld)", (long long)max_candidates);
  if (!d_work || !d_idx || !d_key) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  return lsh_lists_device(lsh_one_set(d_sig, n, ld_sig, n_hash, bands, rows), threshold, top, max_candidates, d_work, work_bytes, d_idx, d_key,
                          static_cast<hipStream_t>(stream));
}

int da_similarity_mh_lsh_knn(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, int n_hash, const uint32_t *seeds, int bands, int rows,
                             double threshold, int top, int64_t max_candidates, int32_t *idx_out, double *val_out) {
  int rc = validate_mh(n, k, n_hash);
  if (rc != DA_OK) return rc;
  if (!residues || !seeds || !idx_out || !val_out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  int64_t total, max_len;
  if ((rc = check_offsets(offsets, n, &total, &max_len)) != DA_OK) return rc;
  if ((rc = lsh_arg_check(n_hash, bands, rows, threshold, max_candidates, &top)) != DA_OK) return rc;
  if ((rc = require_device()) != DA_OK) return rc;
  MhPlanes mh;
  DevBuf work, didx, dkey;
  const StreamDrain drain{nullptr};
  if ((rc = mh.in.upload(residues, offsets, n, total, seeds, n_hash)) != DA_OK) return rc;
  if ((rc = mh.alloc(n, n_hash, false)) != DA_OK || (rc = mh.signatures(k, 0, n_hash)) != DA_OK) return rc;
  const size_t wb = lsh_workspace_bytes(n, bands);
  if ((rc = work.alloc(wb)) != DA_OK || (rc = didx.alloc((size_t)n * (size_t)top * sizeof(int32_t))) != DA_OK ||
      (rc = dkey.alloc((size_t)n * (size_t)top * sizeof(uint16_t))) != DA_OK) return rc;
  if ((rc = lsh_lists_device(lsh_one_set(mh.sig.as<uint32_t>(), n, mh.lds, n_hash, bands, rows), threshold, top, max_candidates, work.p, wb,
                             didx.as<int32_t>(), dkey.as<uint16_t>(), nullptr)) != DA_OK) return rc;
  return topk_to_host(didx, dkey, n, top, mh_code_values(n_hash), idx_out, val_out);
}

int da_dev_lsh_components(const uint32_t *d_sig, int64_t n, int64_t ld_sig, int n_hash, int bands, int rows, double threshold, int64_t max_candidates,
                          void *d_work, size_t work_bytes, int32_t *d_membership, int32_t *d_sizes, int64_t *n_components_out, void *stream) {
  int rc;
  if (n < 0) return fail(DA_ERR_BAD_ARG, "negative shape");
  if (!n_components_out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  *n_components_out = 0;
  if (n == 0) return DA_OK;
  if ((rc = lsh_dev_check(d_sig, n, ld_sig, n_hash, bands, rows, threshold)) != DA_OK) return rc;
  if (max_candidates < 0) return fail(DA_ERR_BAD_ARG, "max_candidates must be >= 0 (got %lld)", (long long)max_candidates);
  if (!d_work || !d_membership) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  return lsh_components_device(lsh_one_set(d_sig, n, ld_sig, n_hash, bands, rows), threshold, max_candidates, d_work, work_bytes, d_membership,
                               d_sizes, n_components_out, static_cast<hipStream_t>(stream));
}

int da_similarity_mh_lsh_components(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, int n_hash, const uint32_t *seeds, int bands,
                                    int rows, double threshold, int64_t max_candidates, int32_t *membership_out, int64_t *n_components_out) {
  int rc = validate_mh(n, k, n_hash);
  if (rc != DA_OK) return rc;
  if (!residues || !seeds || !membership_out || !n_components_out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  *n_components_out = 0;
  int64_t total, max_len;
  if ((rc = check_offsets(offsets, n, &total, &max_len)) != DA_OK) return rc;
  if ((rc = lsh_arg_check(n_hash, bands, rows, threshold, max_candidates)) != DA_OK) return rc;
  if ((rc = require_device()) != DA_OK) return rc;
  MhPlanes mh;
  DevBuf work, member;
  const StreamDrain drain{nullptr};
  if ((rc = mh.in.upload(residues, offsets, n, total, seeds, n_hash)) != DA_OK) return rc;
  if ((rc = mh.alloc(n, n_hash, false)) != DA_OK || (rc = mh.signatures(k, 0, n_hash)) != DA_OK) return rc;
  const size_t wb = lsh_workspace_bytes(n, bands) + components_workspace_bytes(n);
  if ((rc = work.alloc(wb)) != DA_OK || (rc = member.alloc((size_t)n * sizeof(int32_t))) != DA_OK) return rc;
  if ((rc = lsh_components_device(lsh_one_set(mh.sig.as<uint32_t>(), n, mh.lds, n_hash, bands, rows), threshold, max_candidates, work.p, wb,
                                  member.as<int32_t>(), nullptr, n_components_out, nullptr)) != DA_OK) return rc;
  DA_HIP_TRY(hipMemcpy(membership_out, member.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
  return DA_OK;
}

int da_mh_lsh_last_route(int64_t *buckets_out, int64_t *incidences_out, int64_t *verified_pairs_out, int64_t *edges_out) {
  const LshRoute &r = lsh_route();
  if (buckets_out) *buckets_out = r.buckets;
  if (incidences_out) *incidences_out = r.incidences;
  if (verified_pairs_out) *verified_pairs_out = r.verified;
  if (edges_out) *edges_out = r.edges;
  return DA_OK;
}

// ---- MinHash LSH banding for two sets: a resident index probed by query batches (lsh_cross_kernels.hip; the pipelines are above) -------------
}  // extern "C"  (reopened below)
namespace {
// one resident signature matrix of the device calls
int lsh_sig_check(const void *d_sig, int64_t rows_of, int64_t ld, int n_hash, const char *ld_name) {
  if (rows_of < 0) return fail(DA_ERR_BAD_ARG, "negative shape");
  if (n_hash <= 0) return fail(DA_ERR_BAD_NHASH, "%s", da_status_message(DA_ERR_BAD_NHASH));
  if (!d_sig) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (ld < n_hash) return fail(DA_ERR_BAD_ARG, "%s (%lld) < n_hash (%d)", ld_name, (long long)ld, n_hash);
  return DA_OK;
}
int lsh_index_check(const void *d_index, size_t index_bytes, int64_t n, int bands) {
  int rc;
  if ((rc = lsh_elements_check("n", n, bands)) != DA_OK) return rc;
  if (!d_index) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (index_bytes < lsh_index_bytes(n, bands))
    return fail(DA_ERR_BAD_ARG, "lsh: index too small (%zu bytes, %zu needed)", index_bytes, lsh_index_bytes(n, bands));
  return DA_OK;
}
// x, y, the banding and the index of the device calls that run the pipeline
int lsh_cross_dev_check(const void *d_index, size_t index_bytes, const void *d_sig_x, int64_t m, int64_t ld_x, const void *d_sig_y, int64_t n, int64_t ld_y,
                        int n_hash, int bands, int rows, double threshold, int64_t max_candidates, const int *top = nullptr) {
  int rc;
  if (m <= 0 || n <= 0) return fail(DA_ERR_EMPTY_INPUT, "%s", da_status_message(DA_ERR_EMPTY_INPUT));
  if ((rc = lsh_sig_check(d_sig_x, m, ld_x, n_hash, "ld_x")) != DA_OK || (rc = lsh_sig_check(d_sig_y, n, ld_y, n_hash, "ld_y")) != DA_OK) return rc;
  if ((rc = lsh_arg_check(n_hash, bands, rows, threshold, max_candidates, top)) != DA_OK) return rc;
  if ((rc = lsh_elements_check("m", m, bands)) != DA_OK) return rc;
  return lsh_index_check(d_index, index_bytes, n, bands);
}

// The index of resident signatures into d_index (lsh_index_bytes(n, bands) bytes).  Synchronises: the scratch goes back to the cache.
int lsh_index_device(const uint32_t *d_sig, int64_t n, int64_t ld_sig, int bands, int rows, void *d_index, hipStream_t stream) {
  int rc;
  DevBuf scratch;
  const StreamDrain drain{stream};
  if ((rc = scratch.alloc(lsh_index_build_scratch_bytes(n, bands))) != DA_OK) return rc;
  if ((rc = lsh_index_build(d_sig, n, ld_sig, bands, rows, d_index, scratch.p, stream)) != DA_OK) return rc;
  DA_HIP_TRY(hipStreamSynchronize(stream));
  return DA_OK;
}

// what both two-set LSH host calls check before a device is needed: x empty, y empty, k, n_hash, pointers, the offsets of x, then of y, the banding
int lsh_cross_host_validate(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues, const int64_t *y_offsets, int64_t n,
                            int k, int n_hash, const uint32_t *seeds, const void *out1, const void *out2, int bands, int rows, double threshold,
                            int64_t max_candidates, const int *top, int64_t *x_total, int64_t *y_total, bool edge_text = false) {
  int rc;
  if ((rc = validate_mh(m, k > 0 ? k : 1, n_hash > 0 ? n_hash : 1)) != DA_OK || (rc = validate_mh(n, k, n_hash)) != DA_OK) return rc;   // x empty, y empty, k, n_hash
  if (!x_residues || !y_residues || !seeds || !out1 || !out2) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  int64_t max_len;
  if ((rc = check_offsets(x_offsets, m, x_total, &max_len)) != DA_OK || (rc = check_offsets(y_offsets, n, y_total, &max_len)) != DA_OK) return rc;
  return lsh_arg_check(n_hash, bands, rows, threshold, max_candidates, top, edge_text);
}
// The host calls' device side up to the index: both sets uploaded, their signatures, the index of y and the probe workspace.
struct LshCrossHost {
  MhPlanes x, y;
  DevBuf index, work;
  size_t wb = 0;
  int prepare(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, int64_t x_total, const uint8_t *y_residues, const int64_t *y_offsets, int64_t n,
              int64_t y_total, int k, int n_hash, const uint32_t *seeds, int bands, int rows) {
    int rc;
    if ((rc = lsh_elements_check("m", m, bands)) != DA_OK || (rc = lsh_elements_check("n", n, bands)) != DA_OK) return rc;
    if ((rc = x.in.upload(x_residues, x_offsets, m, x_total, seeds, n_hash)) != DA_OK || (rc = y.in.upload(y_residues, y_offsets, n, y_total, seeds, n_hash)) != DA_OK)
      return rc;
    if ((rc = x.alloc(m, n_hash, false)) != DA_OK || (rc = x.signatures(k, 0, n_hash)) != DA_OK || (rc = y.alloc(n, n_hash, false)) != DA_OK ||
        (rc = y.signatures(k, 0, n_hash)) != DA_OK) return rc;
    wb = lsh_cross_workspace_bytes(m, bands);
    if ((rc = index.alloc(lsh_index_bytes(n, bands))) != DA_OK || (rc = work.alloc(wb)) != DA_OK) return rc;
    return lsh_index_device(y.sig.as<uint32_t>(), n, y.lds, bands, rows, index.p, nullptr);
  }
  LshSets sets(int64_t m, int64_t n, int n_hash, int bands, int rows) {
    return LshSets{index.p, x.sig.as<uint32_t>(), m, x.lds, y.sig.as<uint32_t>(), n, y.lds, n_hash, bands, rows};
  }
};
}  // namespace
extern "C" {

size_t da_dev_lsh_index_bytes(int64_t n, int bands) { return lsh_index_bytes(n, bands); }
size_t da_dev_lsh_cross_workspace_bytes(int64_t m, int bands) { return lsh_cross_workspace_bytes(m, bands); }

int da_dev_lsh_index_build(const uint32_t *d_sig_y, int64_t n, int64_t ld_y, int n_hash, int bands, int rows, void *d_index, size_t index_bytes,
                           void *stream) {
  int rc;
  if (n <= 0) return fail(DA_ERR_EMPTY_INPUT, "%s", da_status_message(DA_ERR_EMPTY_INPUT));
  if ((rc = lsh_sig_check(d_sig_y, n, ld_y, n_hash, "ld_y")) != DA_OK || (rc = lsh_arg_check(n_hash, bands, rows, 0.0, 0)) != DA_OK) return rc;
  if ((rc = lsh_index_check(d_index, index_bytes, n, bands)) != DA_OK) return rc;
  return lsh_index_device(d_sig_y, n, ld_y, bands, rows, d_index, static_cast<hipStream_t>(stream));
}

int da_dev_lsh_index_probe(const void *d_index, size_t index_bytes, int64_t n, const uint32_t *d_sig_x, int64_t m, int64_t ld_x, int n_hash, int bands,
                           int rows, int32_t *d_lo, int32_t *d_len, void *stream_v) {
  int rc;
  if (m <= 0 || n <= 0) return fail(DA_ERR_EMPTY_INPUT, "%s", da_status_message(DA_ERR_EMPTY_INPUT));
  if ((rc = lsh_sig_check(d_sig_x, m, ld_x, n_hash, "ld_x")) != DA_OK || (rc = lsh_arg_check(n_hash, bands, rows, 0.0, 0)) != DA_OK) return rc;
  if ((rc = lsh_elements_check("m", m, bands)) != DA_OK || (rc = lsh_index_check(d_index, index_bytes, n, bands)) != DA_OK) return rc;
  if (!d_lo || !d_len) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  DevBuf stats;
  const StreamDrain drain{stream};
  if ((rc = stats.alloc(16)) != DA_OK) return rc;
  int mismatch = 0;
  if ((rc = lsh_index_probe_listed(d_index, n, d_sig_x, m, ld_x, bands, rows, d_lo, d_len, stats.as<uint32_t>(), &mismatch, stream)) != DA_OK) return rc;
  return mismatch ? lsh_index_mismatch(n, bands, rows) : DA_OK;
}

int da_dev_lsh_cross_verify_pairs(const uint32_t *d_sig_x, int64_t m, int64_t ld_x, const uint32_t *d_sig_y, int64_t n, int64_t ld_y, int n_hash, int bands,
                                  int rows, double threshold, const int32_t *d_i, const int32_t *d_j, const int32_t *d_band, int64_t n_triples,
                                  uint16_t *d_count, uint8_t *d_keep, void *stream) {
  int rc;
  if ((rc = lsh_sig_check(d_sig_x, m, ld_x, n_hash, "ld_x")) != DA_OK || (rc = lsh_sig_check(d_sig_y, n, ld_y, n_hash, "ld_y")) != DA_OK) return rc;
  if ((rc = lsh_arg_check(n_hash, bands, rows, threshold, 0)) != DA_OK) return rc;
  if (n_triples < 0) return fail(DA_ERR_BAD_ARG, "negative shape");
  if (n_triples > 0 && (!d_i || !d_j || !d_band || !d_count || !d_keep)) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  return launch_lsh_verify_listed(d_sig_x, m, ld_x, d_sig_y, n, ld_y, n_hash, bands, rows, lsh_c_min(n_hash, threshold), d_i, d_j, d_band, n_triples, d_count,
                                  d_keep, static_cast<hipStream_t>(stream));
}

int da_dev_lsh_cross_edges(const void *d_index, size_t index_bytes, const uint32_t *d_sig_x, int64_t m, int64_t ld_x, const uint32_t *d_sig_y, int64_t n,
                           int64_t ld_y, int n_hash, int bands, int rows, double threshold, int64_t max_candidates, void *d_work, size_t work_bytes,
                           int32_t *d_i, int32_t *d_j, uint16_t *d_count, int64_t capacity, int64_t *n_edges_out, void *stream_v) {
  int rc;
  if ((rc = lsh_cross_dev_check(d_index, index_bytes, d_sig_x, m, ld_x, d_sig_y, n, ld_y, n_hash, bands, rows, threshold, max_candidates)) != DA_OK) return rc;
  if (!n_edges_out || !d_work) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  if (capacity < 0) return fail(DA_ERR_BAD_ARG, "negative capacity");
  if (capacity > 0 && (!d_i || !d_j || !d_count)) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  DevBuf key, val;
  const StreamDrain drain{stream};
  int64_t edges = 0;
  if ((rc = lsh_edges_device(LshSets{d_index, d_sig_x, m, ld_x, d_sig_y, n, ld_y, n_hash, bands, rows}, threshold, max_candidates, d_work, work_bytes, key, val,
                             &edges, stream)) != DA_OK) return rc;
  if ((rc = launch_lsh_split(key.as<uint64_t>(), val.as<uint16_t>(), std::min(edges, capacity), d_i, d_j, d_count, stream)) != DA_OK) return rc;
  DA_HIP_TRY(hipStreamSynchronize(stream));
  *n_edges_out = edges;
  return DA_OK;
}

int da_dev_lsh_cross_topk(const void *d_index, size_t index_bytes, const uint32_t *d_sig_x, int64_t m, int64_t ld_x, const uint32_t *d_sig_y, int64_t n,
                          int64_t ld_y, int n_hash, int bands, int rows, double threshold, int top, int64_t max_candidates, void *d_work, size_t work_bytes,
                          int32_t *d_idx, uint16_t *d_key, void *stream) {
  int rc;
  if ((rc = lsh_cross_dev_check(d_index, index_bytes, d_sig_x, m, ld_x, d_sig_y, n, ld_y, n_hash, bands, rows, threshold, max_candidates, &top)) != DA_OK)
    return rc;
  if (!d_work || !d_idx || !d_key) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  return lsh_lists_device(LshSets{d_index, d_sig_x, m, ld_x, d_sig_y, n, ld_y, n_hash, bands, rows}, threshold, top, max_candidates, d_work, work_bytes, d_idx,
                          d_key, static_cast<hipStream_t>(stream));
}

int da_similarity_mh_lsh_cross_edges_begin(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues,
                                           const int64_t *y_offsets, int64_t n, int k, int n_hash, const uint32_t *seeds, int bands, int rows,
                                           double threshold, int64_t max_candidates, da_edges **handle_out, int64_t *n_edges_out) {
  int rc;
  int64_t x_total, y_total;
  if ((rc = lsh_cross_host_validate(x_residues, x_offsets, m, y_residues, y_offsets, n, k, n_hash, seeds, handle_out, n_edges_out, bands, rows, threshold,
                                    max_candidates, nullptr, &x_total, &y_total)) != DA_OK) return rc;
  *handle_out = nullptr;
  if ((rc = require_device()) != DA_OK) return rc;
  LshCrossHost h;
  DevBuf key, val;
  const StreamDrain drain{nullptr};
  if ((rc = h.prepare(x_residues, x_offsets, m, x_total, y_residues, y_offsets, n, y_total, k, n_hash, seeds, bands, rows)) != DA_OK) return rc;
  int64_t edges = 0;
  if ((rc = lsh_edges_device(h.sets(m, n, n_hash, bands, rows), threshold, max_candidates, h.work.p, h.wb, key, val, &edges, nullptr)) != DA_OK) return rc;
  std::unique_ptr<da_edges> out(new da_edges);
  std::vector<uint64_t> hk((size_t)edges);
  std::vector<uint16_t> hv((size_t)edges);
  if (edges > 0) {
    DA_HIP_TRY(hipMemcpy(hk.data(), key.p, (size_t)edges * 8, hipMemcpyDeviceToHost));
    DA_HIP_TRY(hipMemcpy(hv.data(), val.p, (size_t)edges * 2, hipMemcpyDeviceToHost));
  }
  const std::vector<double> values = mh_code_values(n_hash);
  EdgeSet &es = out->es;
  es.threshold = threshold;
  es.i.resize((size_t)edges); es.j.resize((size_t)edges); es.w.resize((size_t)edges);
  for (size_t e = 0; e < (size_t)edges; ++e) {
    es.i[e] = (int32_t)(hk[e] >> 32);
    es.j[e] = (int32_t)(hk[e] & 0xFFFFFFFFull);
    es.w[e] = values[hv[e]];
  }
  out->n_edges = edges;
  *n_edges_out = edges;
  *handle_out = out.release();
  return DA_OK;
}

int da_similarity_mh_lsh_cross_topk(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues, const int64_t *y_offsets,
                                    int64_t n, int k, int n_hash, const uint32_t *seeds, int bands, int rows, double threshold, int top,
                                    int64_t max_candidates, int32_t *idx_out, double *val_out) {
  int rc;
  int64_t x_total, y_total;
  if ((rc = lsh_cross_host_validate(x_residues, x_offsets, m, y_residues, y_offsets, n, k, n_hash, seeds, idx_out, val_out, bands, rows, threshold,
                                    max_candidates, &top, &x_total, &y_total)) != DA_OK) return rc;
  if ((rc = require_device()) != DA_OK) return rc;
  LshCrossHost h;
  DevBuf didx, dkey;
  const StreamDrain drain{nullptr};
  if ((rc = h.prepare(x_residues, x_offsets, m, x_total, y_residues, y_offsets, n, y_total, k, n_hash, seeds, bands, rows)) != DA_OK) return rc;
  if ((rc = didx.alloc((size_t)m * (size_t)top * sizeof(int32_t))) != DA_OK || (rc = dkey.alloc((size_t)m * (size_t)top * sizeof(uint16_t))) != DA_OK) return rc;
  if ((rc = lsh_lists_device(h.sets(m, n, n_hash, bands, rows), threshold, top, max_candidates, h.work.p, h.wb, didx.as<int32_t>(), dkey.as<uint16_t>(),
                             nullptr)) != DA_OK) return rc;
  return topk_to_host(didx, dkey, m, top, mh_code_values(n_hash), idx_out, val_out);
}

// ---- NW identity on MinHash LSH candidates (nw_lsh_kernels.hip): the LSH back end's sorted candidate list scored by alignment --------------
}  // extern "C"  (reopened below)
namespace {
struct NwLshRoute { int64_t buckets = 0, incidences = 0, verified = 0, aligned = 0, shorts = 0, longs = 0, edges = 0; };
NwLshRoute &nw_lsh_route() { static thread_local NwLshRoute r; return r; }

// min_matches[length], length 0 .. 2048 (two sequences of 1024 residues and no diagonal step): the smallest matches > 0 whose weight --
// the divide the host entries use for the weights -- reaches the threshold, length + 1 when none does.  The weight grows with matches.
constexpr int NWL_TABLE_LEN = 2049;
std::vector<int32_t> nwl_min_matches(double threshold) {
  std::vector<int32_t> t((size_t)NWL_TABLE_LEN);
  for (int len = 0; len < NWL_TABLE_LEN; ++len) {
    int lo = 1, hi = len + 1;                                // the answer is in [lo, hi]
    while (lo < hi) {
      const int mid = lo + (hi - lo) / 2;
      if ((double)mid / (double)len >= threshold) hi = mid; else lo = mid + 1;
    }
    t[(size_t)len] = lo;
  }
  return t;
}
int nwl_threshold_check(double threshold, double mh_threshold) {
  if (!(threshold >= 0.0 && threshold <= 1.0)) return fail(DA_ERR_BAD_ARG, "threshold must be in [0, 1]");
  if (!(mh_threshold >= 0.0 && mh_threshold <= 1.0)) return fail(DA_ERR_BAD_ARG, "mh_threshold must be in [0, 1]");
  return DA_OK;
}
// the encoded sequences the pairs index: i numbers x, j numbers y (one set: the same buffers)
struct NwlSeqs {
  const uint8_t *x_codes; const int64_t *x_off; int64_t m;
  const uint8_t *y_codes; const int64_t *y_off; int64_t n;
};
// The candidates of lsh_edges_device at mh_threshold and their (matches, length), what the edge list and the lists share: the sorted list
// unpacked into ci / cj, the rescore into mt / ln (cand entries each).  Sets the route's counts; a refused candidate fails the call.
struct NwlScored {
  DevBuf key, val, work, ci, cj, mt, ln;                    // key / val / work: read by launches still in flight when lsh_nw_scored returns
  int64_t cand = 0;
};
int lsh_nw_scored(const LshSets &s, const NwlSeqs &q, double mh_threshold, int64_t max_candidates, void *d_work, size_t work_bytes, int matrix_id,
                  int gap_open, int gap_ext, NwlScored &sc, hipStream_t stream) {
  int rc;
  DevBuf &key = sc.key, &work = sc.work;
  NwLshRoute &route = nw_lsh_route();
  route = NwLshRoute();
  if ((rc = lsh_edges_device(s, mh_threshold, max_candidates, d_work, work_bytes, key, sc.val, &sc.cand, stream)) != DA_OK) return rc;
  const LshRoute &lr = lsh_route();
  route.buckets = lr.buckets; route.incidences = lr.incidences; route.verified = lr.verified; route.aligned = sc.cand;
  const int64_t cand = sc.cand;
  if (cand == 0) return DA_OK;
  const size_t ib = (size_t)cand * sizeof(int32_t);
  // the decision words of the short pairs in flight: what the budget (DYNAALIGN_BLOCK_BYTES, or half of the free memory) leaves, one wavefront at least
  const size_t fixed_b = nw_rescore_fixed_bytes(cand), full_b = nw_rescore_workspace_bytes(cand, false), min_b = nw_rescore_workspace_bytes(cand, true);
  const size_t wb = std::max(min_b, std::min(full_b, fixed_b + block_budget()));
  if ((rc = sc.ci.alloc(ib)) != DA_OK || (rc = sc.cj.alloc(ib)) != DA_OK || (rc = sc.mt.alloc(ib)) != DA_OK || (rc = sc.ln.alloc(ib)) != DA_OK ||
      (rc = work.alloc(wb)) != DA_OK) return rc;
  if ((rc = launch_nwl_split(key.as<uint64_t>(), cand, sc.ci.as<int32_t>(), sc.cj.as<int32_t>(), stream)) != DA_OK) return rc;
  int64_t counts[3] = {0, 0, 0};
  if ((rc = launch_nw_rescore(q.x_codes, q.x_off, q.m, q.y_codes, q.y_off, q.n, sc.ci.as<int32_t>(), sc.cj.as<int32_t>(), cand, matrix_id, gap_open, gap_ext,
                              sc.mt.as<int32_t>(), sc.ln.as<int32_t>(), work.p, wb, counts, stream)) != DA_OK) return rc;
  route.shorts = counts[0]; route.longs = counts[1];
  if (counts[2] > 0)
    return fail(DA_ERR_UNSUPPORTED, "nw lsh: %lld candidate pairs have an empty sequence or one over 1024 residues", (long long)counts[2]);
  return DA_OK;
}
// The edge pipeline on resident signatures and resident encoded sequences: the scored candidates, the verdicts, and the kept entries -- the
// first min(capacity, kept) of them -- in d_i / d_j / d_matches / d_length.
// own: four buffers to allocate for the whole list instead (the host entries).  Synchronises the stream.
int lsh_nw_edges_device(const LshSets &s, const NwlSeqs &q, double mh_threshold, int64_t max_candidates, void *d_work, size_t work_bytes, int matrix_id,
                        int gap_open, int gap_ext, double threshold, int32_t *d_i, int32_t *d_j, int32_t *d_matches, int32_t *d_length, int64_t capacity,
                        int64_t *n_edges_out, hipStream_t stream, DevBuf *own = nullptr) {
  int rc;
  NwlScored sc;
  DevBuf keep, ckept, coff, temp, table;
  const StreamDrain drain{stream};
  NwLshRoute &route = nw_lsh_route();
  *n_edges_out = 0;
  if ((rc = lsh_nw_scored(s, q, mh_threshold, max_candidates, d_work, work_bytes, matrix_id, gap_open, gap_ext, sc, stream)) != DA_OK) return rc;
  const int64_t cand = sc.cand;
  if (cand == 0) return DA_OK;
  const std::vector<int32_t> min_matches = nwl_min_matches(threshold);
  const int64_t chunks = ceil_div(cand, 64);
  const size_t scan_b = nwl_keep_scan_bytes(cand);
  if ((rc = keep.alloc((size_t)cand)) != DA_OK || (rc = ckept.alloc((size_t)(chunks + 1) * 8)) != DA_OK || (rc = coff.alloc((size_t)(chunks + 1) * 8)) != DA_OK ||
      (rc = temp.alloc(scan_b)) != DA_OK || (rc = table.alloc((size_t)NWL_TABLE_LEN * sizeof(int32_t))) != DA_OK) return rc;
  DA_HIP_TRY(hipMemcpy(table.p, min_matches.data(), (size_t)NWL_TABLE_LEN * sizeof(int32_t), hipMemcpyHostToDevice));
  if ((rc = launch_nwl_keep(sc.mt.as<int32_t>(), sc.ln.as<int32_t>(), cand, table.as<int32_t>(), NWL_TABLE_LEN, keep.as<uint8_t>(), ckept.as<int64_t>(),
                            coff.as<int64_t>(), temp.p, scan_b, stream)) != DA_OK) return rc;
  int64_t kept = 0;
  DA_HIP_TRY(hipMemcpyAsync(&kept, coff.as<int64_t>() + chunks, 8, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipStreamSynchronize(stream));
  if (own) {                                                // a host entry: the whole list, in buffers sized now that its length is known
    for (int f = 0; f < 4; ++f)
      if ((rc = own[f].alloc((size_t)std::max<int64_t>(kept, 1) * sizeof(int32_t))) != DA_OK) return rc;
    d_i = own[0].as<int32_t>(); d_j = own[1].as<int32_t>(); d_matches = own[2].as<int32_t>(); d_length = own[3].as<int32_t>();
    capacity = kept;
  }
  if ((rc = launch_nwl_emit(sc.ci.as<int32_t>(), sc.cj.as<int32_t>(), sc.mt.as<int32_t>(), sc.ln.as<int32_t>(), keep.as<uint8_t>(), coff.as<int64_t>(), cand,
                            std::min(capacity, kept), d_i, d_j, d_matches, d_length, stream)) != DA_OK) return rc;
  DA_HIP_TRY(hipStreamSynchronize(stream));
  route.edges = kept;
  *n_edges_out = kept;
  return DA_OK;
}
// what the device entries check of the sequences, the scoring and the outputs
int lsh_nw_dev_check(const NwlSeqs &q, int matrix_id, double threshold, const void *d_work, const void *d_i, const void *d_j, const void *d_matches,
                     const void *d_length, int64_t capacity, const int64_t *n_edges_out) {
  if (!q.x_codes || !q.x_off || !q.y_codes || !q.y_off) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (!matrix_table_host(matrix_id)) return fail(DA_ERR_BAD_ARG, "matrix id %d out of range", matrix_id);
  if (!(threshold >= 0.0 && threshold <= 1.0)) return fail(DA_ERR_BAD_ARG, "threshold must be in [0, 1]");
  if (!n_edges_out || !d_work) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  if (capacity < 0) return fail(DA_ERR_BAD_ARG, "negative capacity");
  if (capacity > 0 && (!d_i || !d_j || !d_matches || !d_length)) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  return DA_OK;
}
// the kept list of a host entry: the pipeline with buffers of its own, the lists copied out, the weights divided here
int lsh_nw_edges_to_host(const LshSets &s, const NwlSeqs &q, double mh_threshold, int64_t max_candidates, void *d_work, size_t work_bytes, int matrix_id,
                         int gap_open, int gap_ext, double threshold, da_edges **handle_out, int64_t *n_edges_out) {
  int rc;
  int64_t edges = 0;
  DevBuf own[4];
  if ((rc = lsh_nw_edges_device(s, q, mh_threshold, max_candidates, d_work, work_bytes, matrix_id, gap_open, gap_ext, threshold, nullptr, nullptr, nullptr,
                                nullptr, 0, &edges, nullptr, own)) != DA_OK) return rc;
  std::unique_ptr<da_edges> h(new da_edges);
  EdgeSet &es = h->es;
  es.threshold = threshold;
  es.i.resize((size_t)edges); es.j.resize((size_t)edges); es.w.resize((size_t)edges);
  std::vector<int32_t> hm((size_t)edges), hl((size_t)edges);
  if (edges > 0) {
    const size_t ib = (size_t)edges * sizeof(int32_t);
    DA_HIP_TRY(hipMemcpy(es.i.data(), own[0].p, ib, hipMemcpyDeviceToHost));
    DA_HIP_TRY(hipMemcpy(es.j.data(), own[1].p, ib, hipMemcpyDeviceToHost));
    DA_HIP_TRY(hipMemcpy(hm.data(), own[2].p, ib, hipMemcpyDeviceToHost));
    DA_HIP_TRY(hipMemcpy(hl.data(), own[3].p, ib, hipMemcpyDeviceToHost));
  }
  for (size_t e = 0; e < (size_t)edges; ++e) es.w[e] = (double)hm[e] / (double)hl[e];
  h->n_edges = edges;
  *n_edges_out = edges;
  *handle_out = h.release();
  return DA_OK;
}
// the NW checks of the host entries behind the LSH ones: the residues, no empty sequence, the longest sequence
int nwl_host_lengths(const char *what, const int64_t *off, int64_t count) {
  for (int64_t i = 0; i < count; ++i)
    if (off[i + 1] == off[i])
      return fail(DA_ERR_UNSUPPORTED, "sequence %lld%s is empty: its similarities are 0/0 = NaN, which no threshold orders", (long long)(i + 1), what);
  for (int64_t i = 0; i < count; ++i)
    if (off[i + 1] - off[i] > 1024)
      return fail(DA_ERR_UNSUPPORTED, "the alignment kernels take sequences up to 1024 residues (sequence %lld%s: %lld)", (long long)(i + 1), what,
                  (long long)(off[i + 1] - off[i]));
  return DA_OK;
}
// the residues of an uploaded set encoded for the DP
int nwl_encode(const DeviceInput &in, int64_t total, DevBuf &codes, DevBuf &bad) {
  int rc;
  if ((rc = codes.alloc((size_t)std::max<int64_t>(total, 1))) != DA_OK || (rc = bad.alloc(sizeof(int32_t))) != DA_OK) return rc;
  DA_HIP_TRY(hipMemsetAsync(bad.p, 0, sizeof(int32_t), nullptr));
  return launch_nw_encode(in.res.as<uint8_t>(), total, codes.as<uint8_t>(), bad.as<int32_t>(), nullptr);
}
}  // namespace
extern "C" {

size_t da_dev_nw_rescore_workspace_bytes(int64_t pairs, int64_t max_len, int minimal) {
  (void)max_len;   // the wavefront kernel stores nothing without ops: only the lane-per-pair kernel's decision words count, whatever the lengths
  return nw_rescore_workspace_bytes(pairs, minimal != 0);
}

int da_dev_nw_rescore_pairs(const uint8_t *d_x_codes, const int64_t *d_x_offsets, int64_t m, const uint8_t *d_y_codes, const int64_t *d_y_offsets,
                            int64_t n, const int32_t *d_i, const int32_t *d_j, int64_t pairs, int matrix_id, int gap_open, int gap_ext,
                            int32_t *d_matches, int32_t *d_length, void *d_work, size_t work_bytes, void *stream_v) {
  if (pairs < 0 || m < 0 || n < 0) return fail(DA_ERR_BAD_ARG, "negative count");
  if (!matrix_table_host(matrix_id)) return fail(DA_ERR_BAD_ARG, "matrix id %d out of range", matrix_id);
  NwLshRoute &route = nw_lsh_route();
  route = NwLshRoute();
  if (pairs == 0) return DA_OK;
  if (!d_x_codes || !d_x_offsets || !d_y_codes || !d_y_offsets || !d_i || !d_j || !d_matches || !d_length) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  int rc;
  if ((rc = require_device()) != DA_OK) return rc;
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  int64_t counts[3] = {0, 0, 0};
  if ((rc = launch_nw_rescore(d_x_codes, d_x_offsets, m, d_y_codes, d_y_offsets, n, d_i, d_j, pairs, matrix_id, gap_open, gap_ext, d_matches, d_length,
                              d_work, work_bytes, counts, stream)) != DA_OK) return rc;
  route.aligned = pairs; route.shorts = counts[0]; route.longs = counts[1];
  return DA_OK;
}

int da_dev_lsh_nw_edges(const uint32_t *d_sig, int64_t n, int64_t ld_sig, int n_hash, int bands, int rows, double mh_threshold, int64_t max_candidates,
                        const uint8_t *d_codes, const int64_t *d_offsets, int matrix_id, int gap_open, int gap_ext, double threshold, void *d_work,
                        size_t work_bytes, int32_t *d_i, int32_t *d_j, int32_t *d_matches, int32_t *d_length, int64_t capacity, int64_t *n_edges_out,
                        void *stream) {
  int rc;
  if (n <= 0) return fail(DA_ERR_EMPTY_INPUT, "%s", da_status_message(DA_ERR_EMPTY_INPUT));
  if ((rc = lsh_dev_check(d_sig, n, ld_sig, n_hash, bands, rows, mh_threshold)) != DA_OK) return rc;
  if (max_candidates < 0) return fail(DA_ERR_BAD_ARG, "max_candidates must be >= 0 (got %lld)", (long long)max_candidates);
  const NwlSeqs q{d_codes, d_offsets, n, d_codes, d_offsets, n};
  if ((rc = lsh_nw_dev_check(q, matrix_id, threshold, d_work, d_i, d_j, d_matches, d_length, capacity, n_edges_out)) != DA_OK) return rc;
  return lsh_nw_edges_device(lsh_one_set(d_sig, n, ld_sig, n_hash, bands, rows), q, mh_threshold, max_candidates, d_work, work_bytes, matrix_id, gap_open,
                             gap_ext, threshold, d_i, d_j, d_matches, d_length, capacity, n_edges_out, static_cast<hipStream_t>(stream));
}

int da_dev_lsh_cross_nw_edges(const void *d_index, size_t index_bytes, const uint32_t *d_sig_x, int64_t m, int64_t ld_x, const uint32_t *d_sig_y, int64_t n,
                              int64_t ld_y, int n_hash, int bands, int rows, double mh_threshold, int64_t max_candidates, const uint8_t *d_x_codes,
                              const int64_t *d_x_offsets, const uint8_t *d_y_codes, const int64_t *d_y_offsets, int matrix_id, int gap_open, int gap_ext,
                              double threshold, void *d_work, size_t work_bytes, int32_t *d_i, int32_t *d_j, int32_t *d_matches, int32_t *d_length,
                              int64_t capacity, int64_t *n_edges_out, void *stream) {
  int rc;
  if ((rc = lsh_cross_dev_check(d_index, index_bytes, d_sig_x, m, ld_x, d_sig_y, n, ld_y, n_hash, bands, rows, mh_threshold, max_candidates)) != DA_OK)
    return rc;
  const NwlSeqs q{d_x_codes, d_x_offsets, m, d_y_codes, d_y_offsets, n};
  if ((rc = lsh_nw_dev_check(q, matrix_id, threshold, d_work, d_i, d_j, d_matches, d_length, capacity, n_edges_out)) != DA_OK) return rc;
  return lsh_nw_edges_device(LshSets{d_index, d_sig_x, m, ld_x, d_sig_y, n, ld_y, n_hash, bands, rows}, q, mh_threshold, max_candidates, d_work, work_bytes,
                             matrix_id, gap_open, gap_ext, threshold, d_i, d_j, d_matches, d_length, capacity, n_edges_out, static_cast<hipStream_t>(stream));
}

int da_similarity_nw_lsh_edges_begin(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, int n_hash, const uint32_t *seeds, int bands,
                                     int rows, double mh_threshold, int64_t max_candidates, const char *matrix_name, int gap_open, int gap_ext,
                                     double threshold, da_edges **handle_out, int64_t *n_edges_out) {
  const int mid = da_matrix_id(matrix_name);               // before anything else, as in similarityNW
  if (mid < 0) return DA_ERR_BAD_MATRIX;
  int rc = validate_mh(n, k, n_hash);
  if (rc != DA_OK) return rc;
  if (!residues || !seeds || !handle_out || !n_edges_out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  *handle_out = nullptr;
  int64_t total, max_len;
  if ((rc = check_offsets(offsets, n, &total, &max_len)) != DA_OK) return rc;
  if ((rc = lsh_arg_check(n_hash, bands, rows, 0.0, max_candidates)) != DA_OK) return rc;   // the two thresholds come behind the NW checks
  if ((rc = nw_validate(residues, offsets, n)) != DA_OK) return rc;
  if ((rc = nwl_host_lengths("", offsets, n)) != DA_OK) return rc;
  if ((rc = nwl_threshold_check(threshold, mh_threshold)) != DA_OK) return rc;
  if ((rc = require_device()) != DA_OK) return rc;
  MhPlanes mh;
  DevBuf work, codes, bad;
  const StreamDrain drain{nullptr};
  if ((rc = mh.in.upload(residues, offsets, n, total, seeds, n_hash)) != DA_OK) return rc;
  if ((rc = mh.alloc(n, n_hash, false)) != DA_OK || (rc = mh.signatures(k, 0, n_hash)) != DA_OK) return rc;
  if ((rc = nwl_encode(mh.in, total, codes, bad)) != DA_OK) return rc;
  const size_t wb = lsh_workspace_bytes(n, bands);
  if ((rc = work.alloc(wb)) != DA_OK) return rc;
  const NwlSeqs q{codes.as<uint8_t>(), mh.in.off.as<int64_t>(), n, codes.as<uint8_t>(), mh.in.off.as<int64_t>(), n};
  return lsh_nw_edges_to_host(lsh_one_set(mh.sig.as<uint32_t>(), n, mh.lds, n_hash, bands, rows), q, mh_threshold, max_candidates, work.p, wb, mid, gap_open,
                              gap_ext, threshold, handle_out, n_edges_out);
}

int da_similarity_nw_lsh_cross_edges_begin(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues,
                                           const int64_t *y_offsets, int64_t n, int k, int n_hash, const uint32_t *seeds, int bands, int rows,
                                           double mh_threshold, int64_t max_candidates, const char *matrix_name, int gap_open, int gap_ext,
                                           double threshold, da_edges **handle_out, int64_t *n_edges_out) {
  const int mid = da_matrix_id(matrix_name);               // before anything else, as in similarityNW
  if (mid < 0) return DA_ERR_BAD_MATRIX;
  int rc;
  int64_t x_total, y_total;
  if ((rc = lsh_cross_host_validate(x_residues, x_offsets, m, y_residues, y_offsets, n, k, n_hash, seeds, handle_out, n_edges_out, bands, rows, 0.0,
                                    max_candidates, nullptr, &x_total, &y_total)) != DA_OK) return rc;
  *handle_out = nullptr;
  if ((rc = nw_cross_validate(x_residues, x_offsets, m, y_residues, y_offsets, n)) != DA_OK) return rc;
  if ((rc = nwl_host_lengths(" of x", x_offsets, m)) != DA_OK || (rc = nwl_host_lengths(" of y", y_offsets, n)) != DA_OK) return rc;
  if ((rc = nwl_threshold_check(threshold, mh_threshold)) != DA_OK) return rc;
  if ((rc = require_device()) != DA_OK) return rc;
  LshCrossHost h;
  DevBuf x_codes, y_codes, x_bad, y_bad;
  const StreamDrain drain{nullptr};
  if ((rc = h.prepare(x_residues, x_offsets, m, x_total, y_residues, y_offsets, n, y_total, k, n_hash, seeds, bands, rows)) != DA_OK) return rc;
  if ((rc = nwl_encode(h.x.in, x_total, x_codes, x_bad)) != DA_OK || (rc = nwl_encode(h.y.in, y_total, y_codes, y_bad)) != DA_OK) return rc;
  const NwlSeqs q{x_codes.as<uint8_t>(), h.x.in.off.as<int64_t>(), m, y_codes.as<uint8_t>(), h.y.in.off.as<int64_t>(), n};
  return lsh_nw_edges_to_host(h.sets(m, n, n_hash, bands, rows), q, mh_threshold, max_candidates, h.work.p, h.wb, mid, gap_open, gap_ext, threshold,
                              handle_out, n_edges_out);
}

int da_nw_lsh_last_route(int64_t *buckets_out, int64_t *incidences_out, int64_t *verified_pairs_out, int64_t *aligned_pairs_out, int64_t *short_pairs_out,
                         int64_t *long_pairs_out, int64_t *edges_out) {
  const NwLshRoute &r = nw_lsh_route();
  if (buckets_out) *buckets_out = r.buckets;
  if (incidences_out) *incidences_out = r.incidences;
  if (verified_pairs_out) *verified_pairs_out = r.verified;
  if (aligned_pairs_out) *aligned_pairs_out = r.aligned;
  if (short_pairs_out) *short_pairs_out = r.shorts;
  if (long_pairs_out) *long_pairs_out = r.longs;
  if (edges_out) *edges_out = r.edges;
  return DA_OK;
}


// ---- NW threshold form for sequences of up to 1024 residues: 32-bit keys (nw_edges_long_kernels.hip) ------------------------------------------
// The value table of the PACK32 codes (matches << 16 | length) of sequences up to max_len residues: the distinct doubles
// (double)matches / (double)length, ascending, and rank[length * (max_len + 1) + matches] = the dense rank of that value.
}  // extern "C"  (reopened below)
namespace {
struct NwValueTable {
  int max_len = 0;
  std::vector<double> values;
  std::vector<uint32_t> rank;   // (2 * max_len + 1) * (max_len + 1) entries; row length = 0 is unused (rank 0)
};
// the table of the last max_len asked for is kept: building it is a sort of up to 2.1e6 doubles
std::shared_ptr<const NwValueTable> nw_value_table(int max_len) {
  static std::mutex mu;
  static std::shared_ptr<const NwValueTable> last;
  std::lock_guard<std::mutex> g(mu);
  if (last && last->max_len == max_len) return last;
  auto t = std::make_shared<NwValueTable>();
  t->max_len = max_len;
  const size_t w = (size_t)max_len + 1;
  std::vector<std::pair<double, uint32_t>> v;
  v.reserve((size_t)(2 * max_len) * w);
  for (int ln = 1; ln <= 2 * max_len; ++ln)
    for (int mt = 0; mt <= std::min(ln, max_len); ++mt)
      v.emplace_back((double)mt / (double)ln, (uint32_t)((size_t)ln * w + (size_t)mt));   // the divide of nw_ratio / nw_code_values
  std::sort(v.begin(), v.end());
  t->rank.assign((size_t)(2 * max_len + 1) * w, 0u);
  for (const auto &e : v) {
    if (t->values.empty() || e.first != t->values.back()) t->values.push_back(e.first);
    t->rank[e.second] = (uint32_t)(t->values.size() - 1);
  }
  last = t;
  return last;
}
}  // namespace
extern "C" {

int da_nw_value_ranks(int max_len, double *values_out, int64_t *n_values_out, uint32_t *rank_out) {
  if (!n_values_out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  if (max_len < 1 || max_len > 1024) return fail(DA_ERR_BAD_ARG, "max_len must be in 1 .. 1024 (got %d)", max_len);
  if ((values_out == nullptr) != (rank_out == nullptr)) return fail(DA_ERR_BAD_ARG, "values_out and rank_out must both be given or both be NULL");
  const auto t = nw_value_table(max_len);
  *n_values_out = (int64_t)t->values.size();
  if (!values_out) return DA_OK;                           // size query
  memcpy(values_out, t->values.data(), t->values.size() * sizeof(double));
  memcpy(rank_out, t->rank.data(), t->rank.size() * sizeof(uint32_t));
  return DA_OK;
}

static int rank_block_check(const void *a, const void *b, int64_t rows, int64_t n, int64_t ld, int64_t nbins, int64_t row_begin, int64_t col_begin) {
  if (rows < 0 || n < 0) return fail(DA_ERR_BAD_ARG, "negative shape");
  if (!a || !b) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (ld < n) return fail(DA_ERR_BAD_ARG, "ld (%lld) < n (%lld)", (long long)ld, (long long)n);
  if (nbins < 1 || nbins > 0x7fffffffLL) return fail(DA_ERR_BAD_ARG, "nbins must be in 1 .. 2^31 - 1 (got %lld)", (long long)nbins);
  if (row_begin < 0 || col_begin < 0) return fail(DA_ERR_BAD_ARG, "negative block origin");
  return DA_OK;
}
int da_dev_nw_codes_to_ranks(const uint32_t *d_codes, int64_t rows, int64_t n, int64_t ld, int max_len, const uint32_t *d_rank, uint32_t *d_out,
                             int64_t ld_out, void *stream) {
  int rc;
  if ((rc = rank_block_check(d_codes, d_rank, rows, n, ld, 1, 0, 0)) != DA_OK) return rc;
  if (!d_out) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (ld_out < n) return fail(DA_ERR_BAD_ARG, "ld (%lld) < n (%lld)", (long long)ld_out, (long long)n);
  if (max_len < 1 || max_len > 1024) return fail(DA_ERR_BAD_ARG, "max_len must be in 1 .. 1024 (got %d)", max_len);
  return launch_nw_codes_to_ranks(d_codes, rows, n, ld, max_len, d_rank, d_out, ld_out, static_cast<hipStream_t>(stream));
}
int da_dev_rank_histogram(const uint32_t *d_keys, int64_t rows, int64_t n, int64_t ld, int64_t nbins, uint64_t *d_hist, int triangle,
                          int64_t row_begin, int64_t col_begin, void *stream) {
  int rc;
  if ((rc = rank_block_check(d_keys, d_hist, rows, n, ld, nbins, row_begin, col_begin)) != DA_OK) return rc;
  return launch_rank_histogram(d_keys, rows, n, ld, nbins, reinterpret_cast<unsigned long long *>(d_hist), triangle != 0, row_begin, col_begin,
                               static_cast<hipStream_t>(stream));
}
int da_dev_threshold_ranks_count(const uint32_t *d_keys, int64_t rows, int64_t n, int64_t ld, uint32_t r_min, int64_t nbins, int triangle,
                                 int64_t row_begin, int64_t col_begin, int64_t *d_rowptr, void *d_work, size_t work_bytes, void *stream) {
  int rc;
  if ((rc = rank_block_check(d_keys, d_rowptr, rows, n, ld, nbins, row_begin, col_begin)) != DA_OK) return rc;
  if (!d_work) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  return launch_threshold_ranks_count(d_keys, rows, n, ld, r_min, nbins, triangle != 0, row_begin, col_begin, d_rowptr, d_work, work_bytes,
                                      static_cast<hipStream_t>(stream));
}
int da_dev_threshold_ranks_emit(const uint32_t *d_keys, int64_t rows, int64_t n, int64_t ld, uint32_t r_min, int64_t nbins, int triangle,
                                int64_t row_begin, int64_t col_begin, const int64_t *d_rowptr, int32_t *d_j, uint32_t *d_key_out, int64_t capacity,
                                void *stream) {
  int rc;
  if ((rc = rank_block_check(d_keys, d_rowptr, rows, n, ld, nbins, row_begin, col_begin)) != DA_OK) return rc;
  if (capacity < 0) return fail(DA_ERR_BAD_ARG, "negative capacity");
  if (capacity > 0 && (!d_j || !d_key_out)) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  return launch_threshold_ranks_emit(d_keys, rows, n, ld, r_min, nbins, triangle != 0, row_begin, col_begin, d_rowptr, d_j, d_key_out, capacity,
                                     static_cast<hipStream_t>(stream));
}

// exact top-k per row of a block of value ranks (topk_kernels.hip: k_topk_ranks), and the same with every row's own column left out
int da_dev_topk_ranks(const uint32_t *d_keys, int64_t rows, int64_t n, int64_t ld, int64_t nbins, int top, int32_t *d_idx, uint32_t *d_key_out,
                      int64_t ld_out, void *stream) {
  int rc;
  if ((rc = rank_block_check(d_keys, d_idx, rows, n, ld, nbins, 0, 0)) != DA_OK) return rc;
  if (!d_key_out) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (rows == 0) return DA_OK;
  if (top >= 1 && top <= n && top <= DA_TOPK_MAX && ld_out < top) return fail(DA_ERR_BAD_ARG, "ld_out (%lld) < top (%d)", (long long)ld_out, top);
  return launch_topk_ranks(d_keys, rows, n, ld, nbins, top, d_idx, ld_out, d_key_out, ld_out, static_cast<hipStream_t>(stream));
}
int da_dev_topk_ranks_self(const uint32_t *d_keys, int64_t rows, int64_t n, int64_t ld, int64_t nbins, int top, int64_t self_col0, int32_t *d_idx,
                           uint32_t *d_key_out, int64_t ld_out, uint32_t *d_self_key, void *stream) {
  int rc;
  if ((rc = rank_block_check(d_keys, d_idx, rows, n, ld, nbins, 0, 0)) != DA_OK) return rc;
  if (!d_key_out) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (rows == 0) return DA_OK;
  if (top >= 1 && top <= n - 1 && top <= DA_TOPK_MAX && ld_out < top) return fail(DA_ERR_BAD_ARG, "ld_out (%lld) < top (%d)", (long long)ld_out, top);
  return launch_topk_ranks_self(d_keys, rows, n, ld, nbins, top, self_col0, d_idx, ld_out, d_key_out, ld_out, d_self_key,
                                static_cast<hipStream_t>(stream));
}

}  // extern "C"  (reopened below)
namespace {
// The scratch block of an NW problem on value ranks, and what fills it.  square: the problem is the n x n matrix of one set (m == n) and a
// block holds rows [b0, b1) against columns [b0, n); otherwise it is the m x n rectangle.  compute(b0, b1, c0, d, ld, whole) writes the
// PACK32 codes of rows [b0, b1), columns from c0 on, to d (`whole`: the block is the entire square -- the symmetric sweep fills it at half
// the DP).  Rows per block: a multiple of 8 (the tile of the wavefront kernels), at least 8 -- a row of long sequences is a lot of DP, so the
// blocks follow the budget closely instead of block_rows' 128-row units.
typedef std::function<int(int64_t, int64_t, int64_t, void *, int64_t, bool)> RankCompute;
struct RankBlocks {
  const std::shared_ptr<const NwValueTable> table;
  const std::vector<double> &values;          // ascending: a rank indexes it
  const RankCompute compute;
  const hipStream_t stream;
  const bool square;
  const int max_len;
  const int64_t n, ld, blk;
  const bool whole;
  DevBuf d, drank;
  RankBlocks(int64_t m, int64_t n_, bool square_, int max_len_, const RankCompute &compute_, hipStream_t stream_)
      : table(nw_value_table(max_len_)), values(table->values), compute(compute_), stream(stream_), square(square_), max_len(max_len_), n(n_),
        ld((n_ + 3) / 4 * 4), blk(std::min(std::max<int64_t>((int64_t)(block_budget() / ((size_t)ld * sizeof(uint32_t))) / 8 * 8, 8), m)),
        whole(square_ && blk >= m) {}
  int init() {
    int rc;
    if ((rc = d.alloc((size_t)blk * (size_t)ld * sizeof(uint32_t))) != DA_OK || (rc = drank.alloc(table->rank.size() * sizeof(uint32_t))) != DA_OK) return rc;
    DA_HIP_TRY(hipMemcpyAsync(drank.p, table->rank.data(), table->rank.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    return DA_OK;
  }
  int64_t bins() const { return (int64_t)values.size(); }
  int64_t c0(int64_t b0) const { return square ? b0 : 0; }
  int ranks_of(int64_t b0, int64_t b1) {      // the block's codes, then its ranks in place
    int rc;
    if ((rc = compute(b0, b1, c0(b0), d.p, ld, whole)) != DA_OK) return rc;
    return launch_nw_codes_to_ranks(d.as<uint32_t>(), b1 - b0, n - c0(b0), ld, max_len, drank.as<uint32_t>(), d.as<uint32_t>(), ld, stream);
  }
  // hist[rank] += occurrences in the block -- of the strict upper triangle when the problem is square
  int histogram(int64_t b0, int64_t b1, unsigned long long *d_hist) {
    return launch_rank_histogram(d.as<uint32_t>(), b1 - b0, n - c0(b0), ld, bins(), d_hist, square, b0, c0(b0), stream);
  }
};
// ... as the keys of threshold_blocks: the edges take the rectangle, or the triangle WITH the diagonal; w = values[rank]
struct RankKeys : RankBlocks {
  typedef uint32_t Key;
  uint32_t r_min = 1;
  using RankBlocks::RankBlocks;
  int produce(int64_t b0, int64_t b1) { return ranks_of(b0, b1); }
  int quantile(const std::vector<uint64_t> &h, double p, double *thr) const {   // ranks ARE the ascending value order
    return da_quantile_type7(h.data(), values.data(), (int)bins(), p, thr);
  }
  // kept: value >= threshold and value > 0, i.e. rank >= max(r_thr, 1), r_thr the smallest rank whose value is >= threshold
  int set_threshold(double thr) {
    r_min = (uint32_t)std::max<int64_t>(std::lower_bound(values.begin(), values.end(), thr) - values.begin(), 1);
    return DA_OK;
  }
  int count(int64_t b0, int64_t b1, int64_t *d_rowptr, void *d_work, size_t work_bytes) {
    return launch_threshold_ranks_count(d.as<uint32_t>(), b1 - b0, n - c0(b0), ld, r_min, bins(), square, b0, c0(b0), d_rowptr, d_work, work_bytes, stream);
  }
  int emit(int64_t b0, int64_t b1, const int64_t *d_rowptr, int32_t *d_j, uint32_t *d_key, int64_t capacity) {
    return launch_threshold_ranks_emit(d.as<uint32_t>(), b1 - b0, n - c0(b0), ld, r_min, bins(), square, b0, c0(b0), d_rowptr, d_j, d_key, capacity,
                                       stream);
  }
};
// the PACK32 codes of one set's square: the whole of it by the symmetric sweep (every pair computed once and mirrored), else rows [b0, b1)
// against columns [c0, n)
RankCompute nw_square_codes(const NwCodes &nw, int64_t n, int64_t max_len, int mid, int gap_open, int gap_ext, hipStream_t stream) {
  return [=, &nw](int64_t b0, int64_t b1, int64_t c0, void *d, int64_t ld, bool whole) {
    if (whole)
      return launch_nw(nw.codes.as<uint8_t>(), nw.in.off.as<int64_t>(), n, max_len, mid, gap_open, gap_ext, 0, n, true, DA_OUT_PACK32, d, ld, nullptr, 0,
                       stream);
    return launch_nw_rect(nw.codes.as<uint8_t>(), nw.in.off.as<int64_t>(), n, max_len, mid, gap_open, gap_ext, b0, b1, c0, n, DA_OUT_PACK32, d, ld, stream);
  };
}
}  // namespace
extern "C" {

// da_similarity_nw_edges_begin for sequences of up to 1024 residues: the same validation, the same result
int da_similarity_nw_edges_long_begin(const uint8_t *residues, const int64_t *offsets, int64_t n, const char *matrix_name, int gap_open, int gap_ext,
                                      double thresh_p, da_edges **handle_out, double *threshold_out, int64_t *n_edges_out) {
  return edges_run_handle(handle_out, threshold_out, n_edges_out, [&](bool, EdgeSet &es, int64_t *n_edges) -> int {
    const int mid = da_matrix_id(matrix_name);  // reference :338 -> :190-206, before anything else
    if (mid < 0) return DA_ERR_BAD_MATRIX;
    if (!residues) return fail(DA_ERR_BAD_ARG, "NULL pointer");
    if (n < 2) return fail(DA_ERR_BAD_ARG, "the threshold is a quantile of the strict upper triangle: need >= 2 sequences");
    if (!(thresh_p >= 0.0 && thresh_p <= 1.0)) return fail(DA_ERR_BAD_ARG, "thresh_p must be in [0, 1]");
    int64_t total, max_len;
    int rc;
    if ((rc = check_offsets(offsets, n, &total, &max_len)) != DA_OK) return rc;
    if ((rc = nw_validate(residues, offsets, n)) != DA_OK) return rc;
    for (int64_t i = 0; i < n; ++i)
      if (offsets[i + 1] == offsets[i])
        return fail(DA_ERR_UNSUPPORTED, "sequence %lld is empty: its similarities are 0/0 = NaN and R's quantile() refuses NaN",
                    (long long)(i + 1));
    if (max_len > 1024) return fail(DA_ERR_UNSUPPORTED, "the long NW edge list works on 32-bit value ranks: sequences up to 1024 residues");
    if (n > 0x7ffffff0LL) return fail(DA_ERR_UNSUPPORTED, "too many sequences");
    if ((rc = require_device()) != DA_OK) return rc;
    NwCodes nw;
    if ((rc = nw.upload(residues, offsets, n, total)) != DA_OK) return rc;
    RankKeys keys(n, n, true, (int)max_len, nw_square_codes(nw, n, max_len, mid, gap_open, gap_ext, nullptr), nullptr);
    return edges_to_host(keys, n, thresh_p, true, es, n_edges);
  });
}

// da_similarity_nw_cross_edges_begin for sequences of up to 1024 residues
int da_similarity_nw_cross_edges_long_begin(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues,
                                            const int64_t *y_offsets, int64_t n, const char *matrix_name, int gap_open, int gap_ext, double thresh,
                                            int thresh_is_quantile, da_edges **handle_out, double *threshold_out, int64_t *n_edges_out) {
  return edges_run_handle(handle_out, threshold_out, n_edges_out, [&](bool, EdgeSet &es, int64_t *n_edges) -> int {
    const int mid = da_matrix_id(matrix_name);             // before anything else, as in similarityNW
    if (mid < 0) return DA_ERR_BAD_MATRIX;
    int rc;
    if (m <= 0 || n <= 0) {                                // an empty rectangle: no edges; it has no quantile
      if ((rc = thresh_arg_check(thresh, thresh_is_quantile)) != DA_OK) return rc;
      if (thresh_is_quantile) return fail(DA_ERR_BAD_ARG, "quantile of an empty set");
      es.threshold = thresh;
      *n_edges = 0;
      return DA_OK;
    }
    NwCross c{x_residues, y_residues, x_offsets, y_offsets, m, n, mid, gap_open, gap_ext};
    if ((rc = c.check(true, [&] { return thresh_arg_check(thresh, thresh_is_quantile); }, "a quantile", 1024,
                      "the long NW two-set edge list works on 32-bit value ranks: sequences up to 1024 residues")) != DA_OK) return rc;
    if (m > 0x7ffffff0LL || n > 0x7ffffff0LL) return fail(DA_ERR_UNSUPPORTED, "too many sequences");
    if ((rc = c.upload()) != DA_OK) return rc;
    RankKeys keys(m, n, false, (int)c.max_len, [&](int64_t b0, int64_t b1, int64_t, void *d, int64_t ld, bool) {
      return c.rows(b0, b1, DA_OUT_PACK32, d, ld, nullptr);
    }, nullptr);
    return edges_to_host(keys, m, thresh, thresh_is_quantile != 0, es, n_edges);
  });
}

// ---- nearest-neighbour lists and top-k for sequences of up to 1024 residues: the selection on 32-bit value ranks (k_topk_ranks) -----------------
}  // extern "C"  (reopened below)
namespace {
// Rows [0, m) of the problem `keys` fills, selected block by block: per block the DP (PACK32), the value ranks in place, `top` of every row
// into [m][top] index and rank buffers; then idx as it is, val = values[rank] -- the library's divide bit for bit, as in the edge path.  self:
// the rows are the square problem's own (all n columns) and a block starting at row b0 runs the self form with self_col0 = b0;
// diag = values[the own column's rank].
int rank_topk_to_host(RankBlocks &keys, int64_t m, int top, bool self, int32_t *idx_out, double *val_out, double *diag_out) {
  const hipStream_t stream = keys.stream;
  const size_t cnt = (size_t)m * (size_t)top;
  DevBuf didx, dkey, dself;
  int rc;
  if ((rc = keys.init()) != DA_OK || (rc = didx.alloc(cnt * sizeof(int32_t))) != DA_OK || (rc = dkey.alloc(cnt * sizeof(uint32_t))) != DA_OK) return rc;
  if (self && (rc = dself.alloc((size_t)m * sizeof(uint32_t))) != DA_OK) return rc;
  for (int64_t b0 = 0; b0 < m; b0 += keys.blk) {
    const int64_t b1 = std::min(m, b0 + keys.blk);
    if ((rc = keys.ranks_of(b0, b1)) != DA_OK) return rc;
    rc = self ? launch_topk_ranks_self(keys.d.as<uint32_t>(), b1 - b0, keys.n, keys.ld, keys.bins(), top, b0, didx.as<int32_t>() + b0 * top, top,
                                       dkey.as<uint32_t>() + b0 * top, top, dself.as<uint32_t>() + b0, stream)
              : launch_topk_ranks(keys.d.as<uint32_t>(), b1 - b0, keys.n, keys.ld, keys.bins(), top, didx.as<int32_t>() + b0 * top, top,
                                  dkey.as<uint32_t>() + b0 * top, top, stream);
    if (rc != DA_OK) return rc;
  }
  DA_HIP_TRY(hipStreamSynchronize(stream));
  DA_HIP_TRY(hipMemcpy(idx_out, didx.p, cnt * sizeof(int32_t), hipMemcpyDeviceToHost));
  const std::vector<double> &values = keys.values;
  std::vector<uint32_t> rk;
  if (val_out) {
    rk.resize(cnt);
    DA_HIP_TRY(hipMemcpy(rk.data(), dkey.p, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t e = 0; e < cnt; ++e) val_out[e] = values[std::min<size_t>(rk[e], values.size() - 1)];
  }
  if (self && diag_out) {
    rk.resize((size_t)m);
    DA_HIP_TRY(hipMemcpy(rk.data(), dself.p, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < m; ++i) diag_out[i] = values[std::min<size_t>(rk[(size_t)i], values.size() - 1)];
  }
  return DA_OK;
}
// the PACK32 codes of FULL rows of one set's square, columns [0, n): the whole of it by the symmetric sweep (every pair computed once and
// mirrored, the diagonal included), else rows [b0, b1) through the rectangle form, where pair (p, q) is calc(seq[min], seq[max]) -- so a
// square cut into blocks computes every pair twice, once in each of its two rows' blocks
RankCompute nw_full_row_codes(const NwCodes &nw, int64_t n, int64_t max_len, int mid, int gap_open, int gap_ext, hipStream_t stream) {
  return [=, &nw](int64_t b0, int64_t b1, int64_t, void *d, int64_t ld, bool) {
    if (b0 == 0 && b1 == n)
      return launch_nw(nw.codes.as<uint8_t>(), nw.in.off.as<int64_t>(), n, max_len, mid, gap_open, gap_ext, 0, n, true, DA_OUT_PACK32, d, ld, nullptr, 0,
                       stream);
    return launch_nw_rect(nw.codes.as<uint8_t>(), nw.in.off.as<int64_t>(), n, max_len, mid, gap_open, gap_ext, b0, b1, 0, n, DA_OUT_PACK32, d, ld, stream);
  };
}
}  // namespace
extern "C" {

// da_similarity_nw_knn for sequences of up to 1024 residues: the same validation, the same result
int da_similarity_nw_knn_long(const uint8_t *residues, const int64_t *offsets, int64_t n, const char *matrix_name, int gap_open, int gap_ext, int top,
                              int32_t *idx_out, double *val_out, double *diag_out) {
  const int mid = da_matrix_id(matrix_name);             // before anything else, as in similarityNW
  if (mid < 0) return DA_ERR_BAD_MATRIX;
  if (!residues || !idx_out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  int rc;
  if ((rc = knn_check(top, n)) != DA_OK) return rc;      // where da_similarity_nw_edges checks n >= 2 and thresh_p
  int64_t total, max_len;
  if ((rc = check_offsets(offsets, n, &total, &max_len)) != DA_OK) return rc;
  if ((rc = nw_validate(residues, offsets, n)) != DA_OK) return rc;
  for (int64_t i = 0; i < n; ++i)
    if (offsets[i + 1] == offsets[i])
      return fail(DA_ERR_UNSUPPORTED, "sequence %lld is empty: its similarities are 0/0 = NaN and a NaN has no place in an order", (long long)(i + 1));
  if (max_len > 1024)
    return fail(DA_ERR_UNSUPPORTED, "the long NW nearest-neighbour lists work on 32-bit value ranks: sequences up to 1024 residues");
  if ((rc = require_device()) != DA_OK) return rc;
  NwCodes nw;
  if ((rc = nw.upload(residues, offsets, n, total)) != DA_OK) return rc;
  // not `square`: a block holds all n columns of its rows
  RankBlocks keys(n, n, false, (int)max_len, nw_full_row_codes(nw, n, max_len, mid, gap_open, gap_ext, nullptr), nullptr);
  return rank_topk_to_host(keys, n, top, true, idx_out, val_out, diag_out);
}

// da_similarity_nw_cross_topk for sequences of up to 1024 residues
int da_similarity_nw_cross_topk_long(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues, const int64_t *y_offsets,
                                     int64_t n, const char *matrix_name, int gap_open, int gap_ext, int top, int32_t *idx_out, double *val_out) {
  const int mid = da_matrix_id(matrix_name);             // before anything else, as in similarityNW
  if (mid < 0) return DA_ERR_BAD_MATRIX;
  if (m <= 0) return DA_OK;                              // no rows: nothing to write
  if (n <= 0) return fail(DA_ERR_BAD_ARG, "top must be in 1 .. n (got top = %d, n = 0)", top);
  NwCross c{x_residues, y_residues, x_offsets, y_offsets, m, n, mid, gap_open, gap_ext};
  int rc;
  if ((rc = c.check(idx_out != nullptr, [&] { return topk_check(top, n); }, "an order", 1024,
                    "the long NW top-k works on 32-bit value ranks: sequences up to 1024 residues")) != DA_OK || (rc = c.upload()) != DA_OK) return rc;
  RankBlocks keys(m, n, false, (int)c.max_len, [&](int64_t b0, int64_t b1, int64_t, void *d, int64_t ld, bool) {
    return c.rows(b0, b1, DA_OUT_PACK32, d, ld, nullptr);
  }, nullptr);
  return rank_topk_to_host(keys, m, top, false, idx_out, val_out, nullptr);
}

// ---- NW-ranked nearest-neighbour lists on MinHash LSH candidates: the scored candidates of lsh_nw_scored, ordered by value rank ----------------
}  // extern "C"  (reopened below)
namespace {
// kept: value >= threshold and value > 0, as in RankKeys::set_threshold
uint32_t nwl_r_min(const std::vector<double> &values, double threshold) {
  return (uint32_t)std::max<int64_t>(std::lower_bound(values.begin(), values.end(), threshold) - values.begin(), 1);
}
// The list pipeline on resident signatures and resident encoded sequences: the scored candidates, their value ranks and keep bytes (one
// set: the diagonal into d_diag_key), the ragged rows -- both directions of every kept pair of one set, the x rows of two sets -- and the
// selection into d_idx / d_key ((m, top), leading dimension top).  Synchronises the stream (totals are read back).
int lsh_nw_lists_device(const LshSets &s, const NwlSeqs &q, double mh_threshold, int64_t max_candidates, void *d_work, size_t work_bytes, int matrix_id,
                        int gap_open, int gap_ext, uint32_t r_min, int top, const uint32_t *d_rank, int max_len, int32_t *d_idx, uint32_t *d_key,
                        uint32_t *d_diag_key, hipStream_t stream) {
  int rc;
  NwlScored sc;
  DevBuf rkey, keep, totals, cursor, ptr, col, val, written, temp;
  const StreamDrain drain{stream};
  const bool both = !s.d_index;
  const int64_t m = s.m;
  if ((rc = lsh_nw_scored(s, q, mh_threshold, max_candidates, d_work, work_bytes, matrix_id, gap_open, gap_ext, sc, stream)) != DA_OK) return rc;
  const int64_t cand = sc.cand;
  if ((rc = rkey.alloc((size_t)cand * sizeof(uint32_t))) != DA_OK || (rc = keep.alloc((size_t)cand)) != DA_OK || (rc = totals.alloc(16)) != DA_OK) return rc;
  if (both) DA_HIP_TRY(hipMemsetAsync(d_diag_key, 0, (size_t)m * sizeof(uint32_t), stream));
  if ((rc = launch_nwl_rank_keys(sc.ci.as<int32_t>(), sc.cj.as<int32_t>(), sc.mt.as<int32_t>(), sc.ln.as<int32_t>(), cand, d_rank, max_len, r_min, both, m,
                                 rkey.as<uint32_t>(), keep.as<uint8_t>(), d_diag_key, totals.as<uint64_t>(), stream)) != DA_OK) return rc;
  uint64_t tot[2] = {0, 0};
  DA_HIP_TRY(hipMemcpyAsync(tot, totals.p, 16, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipStreamSynchronize(stream));
  if (tot[1] > 0)
    return fail(DA_ERR_UNSUPPORTED, "nw lsh: %llu candidate pairs have no rank: refused by the alignment kernels, or longer than the table's max_len = %d",
                (unsigned long long)tot[1], max_len);
  const int64_t entries = (int64_t)(both ? 2 * tot[0] : tot[0]);
  const size_t scan_b = lsh_knn_scan_bytes(m);
  if ((rc = cursor.alloc((size_t)(m + 1) * 8)) != DA_OK || (rc = ptr.alloc((size_t)(m + 1) * 8)) != DA_OK || (rc = col.alloc((size_t)entries * 4)) != DA_OK ||
      (rc = val.alloc((size_t)entries * 4)) != DA_OK || (rc = written.alloc(8)) != DA_OK || (rc = temp.alloc(scan_b)) != DA_OK) return rc;
  if ((rc = launch_nw_knn_entries(sc.ci.as<int32_t>(), sc.cj.as<int32_t>(), cand, rkey.as<uint32_t>(), keep.as<uint8_t>(), m, both, entries, top,
                                  cursor.as<int64_t>(), ptr.as<int64_t>(), col.as<int32_t>(), val.as<uint32_t>(), written.as<uint64_t>(), temp.p, scan_b,
                                  stream)) != DA_OK ||
      (rc = launch_nw_knn_select(ptr.as<int64_t>(), entries, col.as<int32_t>(), val.as<uint32_t>(), m, top, d_idx, top, d_key, top, stream)) != DA_OK)
    return rc;
  uint64_t entries_written = 0;
  DA_HIP_TRY(hipMemcpyAsync(&entries_written, written.p, 8, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipStreamSynchronize(stream));
  nw_lsh_route().edges = (int64_t)entries_written;
  return DA_OK;
}
// what the device list entries check behind the LSH checks
int lsh_nw_lists_dev_check(const NwlSeqs &q, int matrix_id, double threshold, const uint32_t *d_rank, int max_len, const void *d_work, const void *d_idx,
                           const void *d_key, const void *d_diag_key, bool one_set) {
  if (!q.x_codes || !q.x_off || !q.y_codes || !q.y_off) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (!matrix_table_host(matrix_id)) return fail(DA_ERR_BAD_ARG, "matrix id %d out of range", matrix_id);
  if (!(threshold >= 0.0 && threshold <= 1.0)) return fail(DA_ERR_BAD_ARG, "threshold must be in [0, 1]");
  if (max_len < 1 || max_len > 1024) return fail(DA_ERR_BAD_ARG, "max_len must be in 1 .. 1024 (got %d)", max_len);
  if (!d_rank || !d_work || !d_idx || !d_key || (one_set && !d_diag_key)) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  return DA_OK;
}
// a host entry behind its checks: the rank table of the call's longest sequence on the device, the pipeline, idx as it is and
// val = values[rank] -- the library's divide bit for bit, as in rank_topk_to_host
int lsh_nw_lists_to_host(const LshSets &s, const NwlSeqs &q, double mh_threshold, int64_t max_candidates, void *d_work, size_t work_bytes, int matrix_id,
                         int gap_open, int gap_ext, double threshold, int top, int max_len, int32_t *idx_out, double *val_out, double *diag_out) {
  int rc;
  const auto table = nw_value_table(max_len);
  const std::vector<double> &values = table->values;
  const int64_t m = s.m;
  const size_t cnt = (size_t)m * (size_t)top;
  const bool one_set = !s.d_index;
  DevBuf drank, didx, dkey, ddiag;
  if ((rc = drank.alloc(table->rank.size() * sizeof(uint32_t))) != DA_OK || (rc = didx.alloc(cnt * sizeof(int32_t))) != DA_OK ||
      (rc = dkey.alloc(cnt * sizeof(uint32_t))) != DA_OK || (rc = ddiag.alloc((size_t)m * sizeof(uint32_t))) != DA_OK) return rc;
  DA_HIP_TRY(hipMemcpy(drank.p, table->rank.data(), table->rank.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  if ((rc = lsh_nw_lists_device(s, q, mh_threshold, max_candidates, d_work, work_bytes, matrix_id, gap_open, gap_ext, nwl_r_min(values, threshold), top,
                                drank.as<uint32_t>(), max_len, didx.as<int32_t>(), dkey.as<uint32_t>(), ddiag.as<uint32_t>(), nullptr)) != DA_OK) return rc;
  DA_HIP_TRY(hipMemcpy(idx_out, didx.p, cnt * sizeof(int32_t), hipMemcpyDeviceToHost));
  std::vector<uint32_t> rk;
  if (val_out) {
    rk.resize(cnt);
    DA_HIP_TRY(hipMemcpy(rk.data(), dkey.p, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t e = 0; e < cnt; ++e) val_out[e] = values[std::min<size_t>(rk[e], values.size() - 1)];
  }
  if (one_set && diag_out) {
    rk.resize((size_t)m);
    DA_HIP_TRY(hipMemcpy(rk.data(), ddiag.p, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < m; ++i) diag_out[i] = values[std::min<size_t>(rk[(size_t)i], values.size() - 1)];
  }
  return DA_OK;
}
}  // namespace
extern "C" {

int da_dev_nw_knn_select(const int64_t *d_ptr, int64_t nnz, const int32_t *d_col, const uint32_t *d_rank_key, int64_t n, int top, int32_t *d_idx,
                         int64_t ld_idx, uint32_t *d_key, int64_t ld_key, void *stream) {
  if (n <= 0) return fail(DA_ERR_EMPTY_INPUT, "%s", da_status_message(DA_ERR_EMPTY_INPUT));
  if (top < 1 || top > DA_TOPK_MAX) return fail(DA_ERR_BAD_ARG, "top must be in 1 .. %d (got %d)", DA_TOPK_MAX, top);
  if (nnz < 0) return fail(DA_ERR_BAD_ARG, "negative shape");
  if (ld_idx < top || ld_key < top) return fail(DA_ERR_BAD_ARG, "ld (%lld) < top (%d)", (long long)std::min(ld_idx, ld_key), top);
  if (!d_ptr || !d_idx || !d_key || (nnz > 0 && (!d_col || !d_rank_key))) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  return launch_nw_knn_select(d_ptr, nnz, d_col, d_rank_key, n, top, d_idx, ld_idx, d_key, ld_key, static_cast<hipStream_t>(stream));
}

int da_dev_nw_rank_keys(const int32_t *d_i, const int32_t *d_j, const int32_t *d_matches, const int32_t *d_length, int64_t pairs, const uint32_t *d_rank,
                        int max_len, uint32_t r_min, int one_set, int64_t n, uint32_t *d_key, uint8_t *d_keep, uint32_t *d_diag_key, uint64_t *d_totals,
                        void *stream) {
  if (pairs < 0 || n < 0) return fail(DA_ERR_BAD_ARG, "negative count");
  if (max_len < 1 || max_len > 1024) return fail(DA_ERR_BAD_ARG, "max_len must be in 1 .. 1024 (got %d)", max_len);
  if (!d_rank || !d_totals || (one_set && n > 0 && !d_diag_key)) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if (pairs > 0 && (!d_i || !d_j || !d_matches || !d_length || !d_key || !d_keep)) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  return launch_nwl_rank_keys(d_i, d_j, d_matches, d_length, pairs, d_rank, max_len, r_min, one_set != 0, n, d_key, d_keep, d_diag_key, d_totals,
                              static_cast<hipStream_t>(stream));
}

int da_dev_lsh_nw_knn(const uint32_t *d_sig, int64_t n, int64_t ld_sig, int n_hash, int bands, int rows, double mh_threshold, int64_t max_candidates,
                      const uint8_t *d_codes, const int64_t *d_offsets, int matrix_id, int gap_open, int gap_ext, double threshold, int top,
                      const uint32_t *d_rank, int max_len, void *d_work, size_t work_bytes, int32_t *d_idx, uint32_t *d_key, uint32_t *d_diag_key,
                      void *stream) {
  int rc;
  if (n <= 0) return fail(DA_ERR_EMPTY_INPUT, "%s", da_status_message(DA_ERR_EMPTY_INPUT));
  if ((rc = lsh_dev_check(d_sig, n, ld_sig, n_hash, bands, rows, mh_threshold)) != DA_OK) return rc;
  if (max_candidates < 0) return fail(DA_ERR_BAD_ARG, "max_candidates must be >= 0 (got %lld)", (long long)max_candidates);
  if (top < 1 || top > DA_TOPK_MAX) return fail(DA_ERR_BAD_ARG, "top must be in 1 .. %d (got %d)", DA_TOPK_MAX, top);
  const NwlSeqs q{d_codes, d_offsets, n, d_codes, d_offsets, n};
  if ((rc = lsh_nw_lists_dev_check(q, matrix_id, threshold, d_rank, max_len, d_work, d_idx, d_key, d_diag_key, true)) != DA_OK) return rc;
  return lsh_nw_lists_device(lsh_one_set(d_sig, n, ld_sig, n_hash, bands, rows), q, mh_threshold, max_candidates, d_work, work_bytes, matrix_id, gap_open,
                             gap_ext, nwl_r_min(nw_value_table(max_len)->values, threshold), top, d_rank, max_len, d_idx, d_key, d_diag_key,
                             static_cast<hipStream_t>(stream));
}

int da_dev_lsh_cross_nw_topk(const void *d_index, size_t index_bytes, const uint32_t *d_sig_x, int64_t m, int64_t ld_x, const uint32_t *d_sig_y, int64_t n,
                             int64_t ld_y, int n_hash, int bands, int rows, double mh_threshold, int64_t max_candidates, const uint8_t *d_x_codes,
                             const int64_t *d_x_offsets, const uint8_t *d_y_codes, const int64_t *d_y_offsets, int matrix_id, int gap_open, int gap_ext,
                             double threshold, int top, const uint32_t *d_rank, int max_len, void *d_work, size_t work_bytes, int32_t *d_idx,
                             uint32_t *d_key, void *stream) {
  int rc;
  if ((rc = lsh_cross_dev_check(d_index, index_bytes, d_sig_x, m, ld_x, d_sig_y, n, ld_y, n_hash, bands, rows, mh_threshold, max_candidates, &top)) != DA_OK)
    return rc;
  const NwlSeqs q{d_x_codes, d_x_offsets, m, d_y_codes, d_y_offsets, n};
  if ((rc = lsh_nw_lists_dev_check(q, matrix_id, threshold, d_rank, max_len, d_work, d_idx, d_key, nullptr, false)) != DA_OK) return rc;
  return lsh_nw_lists_device(LshSets{d_index, d_sig_x, m, ld_x, d_sig_y, n, ld_y, n_hash, bands, rows}, q, mh_threshold, max_candidates, d_work, work_bytes,
                             matrix_id, gap_open, gap_ext, nwl_r_min(nw_value_table(max_len)->values, threshold), top, d_rank, max_len, d_idx, d_key, nullptr,
                             static_cast<hipStream_t>(stream));
}

int da_similarity_nw_lsh_knn(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, int n_hash, const uint32_t *seeds, int bands, int rows,
                             double mh_threshold, int64_t max_candidates, const char *matrix_name, int gap_open, int gap_ext, double threshold, int top,
                             int32_t *idx_out, double *val_out, double *diag_out) {
  const int mid = da_matrix_id(matrix_name);               // before anything else, as in similarityNW
  if (mid < 0) return DA_ERR_BAD_MATRIX;
  int rc = validate_mh(n, k, n_hash);
  if (rc != DA_OK) return rc;
  if (!residues || !seeds || !idx_out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  int64_t total, max_len;
  if ((rc = check_offsets(offsets, n, &total, &max_len)) != DA_OK) return rc;
  if ((rc = lsh_arg_check(n_hash, bands, rows, 0.0, max_candidates, &top, true)) != DA_OK) return rc;   // the two thresholds come behind the NW checks
  if ((rc = nw_validate(residues, offsets, n)) != DA_OK) return rc;
  if ((rc = nwl_host_lengths("", offsets, n)) != DA_OK) return rc;
  if ((rc = nwl_threshold_check(threshold, mh_threshold)) != DA_OK) return rc;
  if ((rc = require_device()) != DA_OK) return rc;
  MhPlanes mh;
  DevBuf work, codes, bad;
  const StreamDrain drain{nullptr};
  if ((rc = mh.in.upload(residues, offsets, n, total, seeds, n_hash)) != DA_OK) return rc;
  if ((rc = mh.alloc(n, n_hash, false)) != DA_OK || (rc = mh.signatures(k, 0, n_hash)) != DA_OK) return rc;
  if ((rc = nwl_encode(mh.in, total, codes, bad)) != DA_OK) return rc;
  const size_t wb = lsh_workspace_bytes(n, bands);
  if ((rc = work.alloc(wb)) != DA_OK) return rc;
  const NwlSeqs q{codes.as<uint8_t>(), mh.in.off.as<int64_t>(), n, codes.as<uint8_t>(), mh.in.off.as<int64_t>(), n};
  return lsh_nw_lists_to_host(lsh_one_set(mh.sig.as<uint32_t>(), n, mh.lds, n_hash, bands, rows), q, mh_threshold, max_candidates, work.p, wb, mid, gap_open,
                              gap_ext, threshold, top, (int)max_len, idx_out, val_out, diag_out);
}

int da_similarity_nw_lsh_cross_topk(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues, const int64_t *y_offsets,
                                    int64_t n, int k, int n_hash, const uint32_t *seeds, int bands, int rows, double mh_threshold,
                                    int64_t max_candidates, const char *matrix_name, int gap_open, int gap_ext, double threshold, int top,
                                    int32_t *idx_out, double *val_out) {
  const int mid = da_matrix_id(matrix_name);               // before anything else, as in similarityNW
  if (mid < 0) return DA_ERR_BAD_MATRIX;
  int rc;
  int64_t x_total, y_total;
  if ((rc = lsh_cross_host_validate(x_residues, x_offsets, m, y_residues, y_offsets, n, k, n_hash, seeds, idx_out, idx_out, bands, rows, 0.0,
                                    max_candidates, &top, &x_total, &y_total, true)) != DA_OK) return rc;
  if ((rc = nw_cross_validate(x_residues, x_offsets, m, y_residues, y_offsets, n)) != DA_OK) return rc;
  if ((rc = nwl_host_lengths(" of x", x_offsets, m)) != DA_OK || (rc = nwl_host_lengths(" of y", y_offsets, n)) != DA_OK) return rc;
  if ((rc = nwl_threshold_check(threshold, mh_threshold)) != DA_OK) return rc;
  if ((rc = require_device()) != DA_OK) return rc;
  int64_t max_len = 1;
  for (int64_t i = 0; i < m; ++i) max_len = std::max(max_len, x_offsets[i + 1] - x_offsets[i]);
  for (int64_t j = 0; j < n; ++j) max_len = std::max(max_len, y_offsets[j + 1] - y_offsets[j]);
  LshCrossHost h;
  DevBuf x_codes, y_codes, x_bad, y_bad;
  const StreamDrain drain{nullptr};
  if ((rc = h.prepare(x_residues, x_offsets, m, x_total, y_residues, y_offsets, n, y_total, k, n_hash, seeds, bands, rows)) != DA_OK) return rc;
  if ((rc = nwl_encode(h.x.in, x_total, x_codes, x_bad)) != DA_OK || (rc = nwl_encode(h.y.in, y_total, y_codes, y_bad)) != DA_OK) return rc;
  const NwlSeqs q{x_codes.as<uint8_t>(), h.x.in.off.as<int64_t>(), m, y_codes.as<uint8_t>(), h.y.in.off.as<int64_t>(), n};
  return lsh_nw_lists_to_host(h.sets(m, n, n_hash, bands, rows), q, mh_threshold, max_candidates, h.work.p, h.wb, mid, gap_open, gap_ext, threshold, top,
                              (int)max_len, idx_out, val_out, nullptr);
}

// ---- summary statistics without the matrix on the host (reference R/similarity.R:11-34; dynaalign.h) ---------------------------------------
static int extrema_block_check(const void *keys, const void *rec, int64_t rows, int64_t n, int64_t ld, int64_t row_begin, int64_t col_begin) {
  return rank_block_check(keys, rec, rows, n, ld, 1, row_begin, col_begin);
}
int da_dev_upper_extrema(const uint16_t *d_keys, int64_t rows, int64_t n, int64_t ld, const uint16_t *d_rank, int64_t row_begin, int64_t col_begin,
                         da_row_extrema *d_records, void *stream) {
  int rc;
  if ((rc = extrema_block_check(d_keys, d_records, rows, n, ld, row_begin, col_begin)) != DA_OK) return rc;
  return launch_upper_extrema(d_keys, rows, n, ld, d_rank, row_begin, col_begin, d_records, static_cast<hipStream_t>(stream));
}
int da_dev_upper_extrema32(const uint32_t *d_keys, int64_t rows, int64_t n, int64_t ld, int64_t row_begin, int64_t col_begin,
                           da_row_extrema *d_records, void *stream) {
  int rc;
  if ((rc = extrema_block_check(d_keys, d_records, rows, n, ld, row_begin, col_begin)) != DA_OK) return rc;
  return launch_upper_extrema32(d_keys, rows, n, ld, row_begin, col_begin, d_records, static_cast<hipStream_t>(stream));
}
}  // extern "C"  (reopened below)

namespace {
// The host side of the statistics: the histogram of the strict upper triangle over value ranks (values ascending, one bin per distinct
// value) gives the four numbers; the per-row records of k_upper_extrema, rows ascending with GLOBAL columns, give the positions.
struct StatsFold {
  std::vector<da_row_extrema> rec;
  // the records of rows [rec.size(), rec.size() + rows) of the square, as the kernel wrote them for a block whose first column is col_begin
  void add_block(const da_row_extrema *r, int64_t rows, int64_t col_begin) {
    for (int64_t i = 0; i < rows; ++i) {
      da_row_extrema e = r[i];
      if (e.min_col >= 0) e.min_col += (int32_t)col_begin;
      if (e.max_col >= 0) e.max_col += (int32_t)col_begin;
      rec.push_back(e);
    }
  }
  // want_max: positions of the largest rank, else of the smallest.  upper: the first (i, j), i < j, in row-major order holding it.  pair: R's
  // which(S == v, arr.ind = TRUE)[1, ] -- the first position in column-major order over the whole matrix, which by symmetry is (c, r) for
  // the first (r, c) in row-major order among the diagonal and the strict upper triangle: going over the rows, r itself when the diagonal
  // holds v, the row's recorded column when the row's extreme is v.
  bool positions(bool want_max, uint32_t *rank_out, int64_t upper[2], int64_t pair[2]) const {
    bool any = false;
    uint32_t ext = 0;
    for (const da_row_extrema &e : rec) {
      if (e.min_col < 0) continue;
      const uint32_t v = want_max ? e.max_key : e.min_key;
      if (!any || (want_max ? v > ext : v < ext)) { ext = v; any = true; }
    }
    if (!any) return false;
    bool have_upper = false, have_pair = false;
    for (size_t r = 0; r < rec.size() && !(have_upper && have_pair); ++r) {
      const da_row_extrema &e = rec[r];
      const bool row_has = e.min_col >= 0 && (want_max ? e.max_key : e.min_key) == ext;
      const int64_t col = want_max ? e.max_col : e.min_col;
      if (!have_upper && row_has) { upper[0] = (int64_t)r; upper[1] = col; have_upper = true; }
      if (!have_pair) {
        if (e.diag_key != 0xFFFFFFFFu && e.diag_key == ext) { pair[0] = pair[1] = (int64_t)r; have_pair = true; }
        else if (row_has) { pair[0] = col; pair[1] = (int64_t)r; have_pair = true; }
      }
    }
    *rank_out = ext;
    return have_upper && have_pair;
  }
  int finish(const std::vector<uint64_t> &hist, const double *values, int64_t n, da_similarity_stats *out) const {
    int rc;
    da_similarity_stats s;
    memset(&s, 0, sizeof s);
    if ((rc = da_stats_from_histogram(hist.data(), values, (int64_t)hist.size(), &s.mean_similarity, &s.median_similarity, &s.min_similarity,
                                      &s.max_similarity)) != DA_OK) return rc;
    s.pairs = n * (n - 1) / 2;
    uint32_t rmin = 0, rmax = 0;
    if (!positions(false, &rmin, s.least_similar_upper, s.least_similar_pair) || !positions(true, &rmax, s.most_similar_upper, s.most_similar_pair))
      return fail(DA_ERR_HIP, "the extrema pass found no element above the diagonal");
    uint64_t total = 0;
    for (uint64_t h : hist) total += h;
    // the two passes read the same triangle: they must agree on its size and its extremes
    if ((int64_t)total != s.pairs || rmin >= hist.size() || rmax >= hist.size() || values[rmin] != s.min_similarity || values[rmax] != s.max_similarity)
      return fail(DA_ERR_HIP, "statistics mismatch: the histogram holds %llu pairs in [%g, %g], the extrema pass found [%g, %g] over %lld",
                  (unsigned long long)total, s.min_similarity, s.max_similarity, rmin < hist.size() ? values[rmin] : -1.0,
                  rmax < hist.size() ? values[rmax] : -1.0, (long long)s.pairs);
    *out = s;
    return DA_OK;
  }
};

// the records of one block to the host fold (synchronises the stream)
int fold_block(StatsFold &fold, const DevBuf &drec, int64_t rows, int64_t col_begin, hipStream_t stream) {
  std::vector<da_row_extrema> h((size_t)rows);
  DA_HIP_TRY(hipMemcpyAsync(h.data(), drec.p, (size_t)rows * sizeof(da_row_extrema), hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipStreamSynchronize(stream));
  fold.add_block(h.data(), rows, col_begin);
  return DA_OK;
}

// what the two NW calls check, in the order of nw_edges_core (matrix name first, DA_ERR_NO_DEVICE last)
int nw_stats_validate(const uint8_t *residues, const int64_t *offsets, int64_t n, const char *matrix_name, const da_similarity_stats *out,
                      int64_t len_limit, int *mid_out, int64_t *total, int64_t *max_len) {
  const int mid = da_matrix_id(matrix_name);  // reference :338 -> :190-206, before anything else
  if (mid < 0) return DA_ERR_BAD_MATRIX;
  if (!residues || !out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  if (n < 2) return fail(DA_ERR_BAD_ARG, "the statistics are over the strict upper triangle: need >= 2 sequences");
  int rc;
  if ((rc = check_offsets(offsets, n, total, max_len)) != DA_OK) return rc;
  if ((rc = nw_validate(residues, offsets, n)) != DA_OK) return rc;
  for (int64_t i = 0; i < n; ++i)
    if (offsets[i + 1] == offsets[i])
      return fail(DA_ERR_UNSUPPORTED, "sequence %lld is empty: its similarities are 0/0 = NaN and R's median() of them is NA", (long long)(i + 1));
  if (*max_len > len_limit)
    return len_limit == 127 ? fail(DA_ERR_UNSUPPORTED, "the NW statistics work on uint16 codes: sequences up to 127 residues")
                            : fail(DA_ERR_UNSUPPORTED, "the long NW statistics work on 32-bit value ranks: sequences up to 1024 residues");
  if (n > 0x7ffffff0LL) return fail(DA_ERR_UNSUPPORTED, "too many sequences");
  *mid_out = mid;
  return require_device();
}
}  // namespace

extern "C" {

// mh_edges_core's pipeline up to and including the histogram, then the extrema of the same resident count matrix
int da_similarity_mh_stats(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, int n_hash, const uint32_t *seeds,
                           da_similarity_stats *out) {
  int rc = validate_mh(n, k, n_hash);
  if (rc != DA_OK) return rc;
  if (!residues || !seeds || !out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  if (n < 2) return fail(DA_ERR_BAD_ARG, "the statistics are over the strict upper triangle: need >= 2 sequences");
  if (n_hash > 65535) return fail(DA_ERR_UNSUPPORTED, "the compare kernel counts in 16 bits: n_hash <= 65535 (got %d)", n_hash);
  int64_t total, max_len;
  if ((rc = check_offsets(offsets, n, &total, &max_len)) != DA_OK) return rc;
  if (n > 0x7ffffff0LL) return fail(DA_ERR_UNSUPPORTED, "too many sequences");
  if ((rc = require_device()) != DA_OK) return rc;
  MhPlanes mh;
  DevBuf cnt, hist, drec;
  if ((rc = mh.in.upload(residues, offsets, n, total, seeds, n_hash)) != DA_OK) return rc;
  if ((rc = mh.alloc(n, n_hash)) != DA_OK) return rc;
  if ((rc = cnt.alloc((size_t)n * (size_t)n * 2)) != DA_OK) return rc;   // uint16 counts stay on the device
  const int nbins = n_hash + 1;
  if ((rc = hist.alloc((size_t)nbins * 8)) != DA_OK || (rc = drec.alloc((size_t)n * sizeof(da_row_extrema))) != DA_OK) return rc;
  DA_HIP_TRY(hipMemset(hist.p, 0, (size_t)nbins * 8));
  if ((rc = mh.build(k, 0, n_hash)) != DA_OK || (rc = mh.finish()) != DA_OK) return rc;
  if ((rc = launch_mh_compare(mh.planes.as<uint32_t>(), n, n_hash, 0, n, true, DA_OUT_COMPACT, cnt.p, n, nullptr, mh.bits)) != DA_OK)
    return rc;
  if ((rc = launch_upper_histogram(cnt.as<uint16_t>(), n, n, nbins, hist.as<unsigned long long>(), nullptr)) != DA_OK) return rc;
  if ((rc = launch_upper_extrema(cnt.as<uint16_t>(), n, n, n, nullptr, 0, 0, drec.as<da_row_extrema>(), nullptr)) != DA_OK) return rc;
  std::vector<uint64_t> h((size_t)nbins);
  DA_HIP_TRY(hipMemcpy(h.data(), hist.p, (size_t)nbins * 8, hipMemcpyDeviceToHost));
  StatsFold fold;
  if ((rc = fold_block(fold, drec, n, 0, nullptr)) != DA_OK) return rc;
  return fold.finish(h, mh_code_values(n_hash).data(), n, out);      // a count is its own rank
}

// nw_edges_core's pipeline (duplicate collapse and prefix sharing of nw_full_symmetric) up to and including the histogram of the codes;
// bins of equal value are merged on the host (R's median sees values), and the extrema compare through the same code -> rank table
int da_similarity_nw_stats(const uint8_t *residues, const int64_t *offsets, int64_t n, const char *matrix_name, int gap_open, int gap_ext,
                           da_similarity_stats *out) {
  int mid = 0, rc;
  int64_t total = 0, max_len = 0;
  if ((rc = nw_stats_validate(residues, offsets, n, matrix_name, out, 127, &mid, &total, &max_len)) != DA_OK) return rc;
  NwCodes nw;
  DevBuf cnt, hist, drank, drec;
  if ((rc = nw.upload(residues, offsets, n, total)) != DA_OK) return rc;
  if ((rc = cnt.alloc((size_t)n * (size_t)n * 2)) != DA_OK) return rc;      // uint16 codes stay on the device
  const int nbins = (int)((max_len << 8) | (2 * max_len)) + 1;              // matches <= max_len, length <= 2 * max_len
  std::vector<uint16_t> ranks(65536);
  int distinct = 0;
  if ((rc = da_nw_code_ranks((int)max_len, ranks.data(), &distinct)) != DA_OK) return rc;
  if ((rc = hist.alloc((size_t)nbins * 8)) != DA_OK || (rc = drank.alloc(65536 * sizeof(uint16_t))) != DA_OK ||
      (rc = drec.alloc((size_t)n * sizeof(da_row_extrema))) != DA_OK) return rc;
  DA_HIP_TRY(hipMemset(hist.p, 0, (size_t)nbins * 8));
  DA_HIP_TRY(hipMemcpy(drank.p, ranks.data(), 65536 * sizeof(uint16_t), hipMemcpyHostToDevice));
  if ((rc = nw_full_symmetric(nw.codes.as<uint8_t>(), nw.in.off.as<int64_t>(), n, total, max_len, mid, gap_open, gap_ext, DA_OUT_COMPACT,
                              cnt.p, n, nullptr)) != DA_OK) return rc;
  if ((rc = launch_upper_histogram(cnt.as<uint16_t>(), n, n, nbins, hist.as<unsigned long long>(), nullptr)) != DA_OK) return rc;
  if ((rc = launch_upper_extrema(cnt.as<uint16_t>(), n, n, n, drank.as<uint16_t>(), 0, 0, drec.as<da_row_extrema>(), nullptr)) != DA_OK) return rc;
  std::vector<uint64_t> h((size_t)nbins);
  DA_HIP_TRY(hipMemcpy(h.data(), hist.p, (size_t)nbins * 8, hipMemcpyDeviceToHost));
  // codes -> value ranks: one bin per distinct value, ascending (length 0 cannot occur: no empty sequences)
  const std::vector<double> code_values = nw_code_values(nbins, 0.0);
  std::vector<uint64_t> hr((size_t)distinct, 0);
  std::vector<double> values((size_t)distinct, 0.0);
  for (int ln = 1; ln <= 2 * (int)max_len; ++ln)
    for (int mt = 0; mt <= std::min(ln, (int)max_len); ++mt) {
      const int code = (mt << 8) | ln;
      values[ranks[(size_t)code]] = code_values[(size_t)code];
      hr[ranks[(size_t)code]] += h[(size_t)code];
    }
  StatsFold fold;
  if ((rc = fold_block(fold, drec, n, 0, nullptr)) != DA_OK) return rc;
  return fold.finish(hr, values.data(), n, out);
}

}  // extern "C"  (reopened below)
namespace {
// The statistics of a square problem on value ranks: the first pass of the long edge lists (RankBlocks: per block the PACK32 codes, the value
// ranks in place, the histogram of the strict upper triangle) with the extrema of the block behind it and its records taken to the host --
// ONE pass of the producer whatever the number of blocks.
int rank_stats(RankBlocks &keys, int64_t n, da_similarity_stats *out) {
  int rc;
  const hipStream_t stream = keys.stream;
  const int64_t nbins = keys.bins();
  const std::vector<double> &values = keys.values;
  DevBuf hist, drec;
  if ((rc = keys.init()) != DA_OK || (rc = hist.alloc((size_t)nbins * 8)) != DA_OK ||
      (rc = drec.alloc((size_t)keys.blk * sizeof(da_row_extrema))) != DA_OK) return rc;
  DA_HIP_TRY(hipMemsetAsync(hist.p, 0, (size_t)nbins * 8, stream));
  StatsFold fold;
  fold.rec.reserve((size_t)n);
  for (int64_t b0 = 0; b0 < n; b0 += keys.blk) {
    const int64_t b1 = std::min(n, b0 + keys.blk), rows = b1 - b0, c0 = keys.c0(b0);   // rows [b0, b1) against columns [b0, n)
    if ((rc = keys.ranks_of(b0, b1)) != DA_OK || (rc = keys.histogram(b0, b1, hist.as<unsigned long long>())) != DA_OK ||
        (rc = launch_upper_extrema32(keys.d.as<uint32_t>(), rows, n - c0, keys.ld, b0, c0, drec.as<da_row_extrema>(), stream)) != DA_OK ||
        (rc = fold_block(fold, drec, rows, c0, stream)) != DA_OK)
      return rc;
  }
  std::vector<uint64_t> h((size_t)nbins);
  DA_HIP_TRY(hipMemcpyAsync(h.data(), hist.p, (size_t)nbins * 8, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipStreamSynchronize(stream));
  return fold.finish(h, values.data(), n, out);      // ranks ARE the ascending value order
}
}  // namespace
extern "C" {

// the long NW identity's statistics: rank_stats on the symmetric sweep / the row-block DP
int da_similarity_nw_stats_long(const uint8_t *residues, const int64_t *offsets, int64_t n, const char *matrix_name, int gap_open, int gap_ext,
                                da_similarity_stats *out) {
  int mid = 0, rc;
  int64_t total = 0, max_len = 0;
  if ((rc = nw_stats_validate(residues, offsets, n, matrix_name, out, 1024, &mid, &total, &max_len)) != DA_OK) return rc;
  NwCodes nw;
  if ((rc = nw.upload(residues, offsets, n, total)) != DA_OK) return rc;
  RankBlocks keys(n, n, true, (int)max_len, nw_square_codes(nw, n, max_len, mid, gap_open, gap_ext, nullptr), nullptr);
  return rank_stats(keys, n, out);
}

// ---- the exact Jaccard index for sequences of up to 1024 shingle positions (dynaalign.h; jaccard_long_kernels.hip) -------------------------------
// Each call is its short sibling with JaccardSets(1024).  The dense calls take doubles from the device; wherever an order is needed the
// PACK32 codes intersection << 16 | union go through the long NW paths' value ranks: with S the call's largest shingle count (at least 1),
// 1 <= union <= 2 S and intersection <= min(union, S), which is the domain of nw_value_table(S).  A rectangle whose rows and columns are
// the same range is computed by the symmetric form (launch_jaccard_rect_long sees it), so a square that fits one block costs half.
int da_similarity_jaccard_long(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, double *out) {
  JaccardSets js(1024);
  int rc;
  if ((rc = js.check_one(residues, offsets, n, k, out != nullptr)) != DA_OK || (rc = js.build(residues, offsets)) != DA_OK) return rc;
  return rows_to_host(n, 0, n, sizeof(double), out, [&](int64_t b0, int64_t b1, void *d) { return js.rect(b0, b1, 0, n, DA_OUT_F64, d, n, nullptr); });
}

int da_similarity_jaccard_cross_long(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues,
                                     const int64_t *y_offsets, int64_t n, int k, double *out, int column_major) {
  if (k <= 0) return fail(DA_ERR_BAD_K, "%s", da_status_message(DA_ERR_BAD_K));
  if (m <= 0 || n <= 0) return DA_OK;                    // an m x 0 or 0 x n matrix: nothing to write
  JaccardSets js(1024);
  int rc;
  if ((rc = js.check_two(x_residues, x_offsets, m, y_residues, y_offsets, n, k, out != nullptr)) != DA_OK ||
      (rc = js.build(x_residues, x_offsets, y_residues, y_offsets)) != DA_OK) return rc;
  const int64_t rows = column_major ? n : m, cols = column_major ? m : n;
  // J is symmetric: rows of y against columns of x are the transpose, R's column-major NumericMatrix(m, n)
  return rows_to_host(cols, 0, rows, sizeof(double), out, [&](int64_t b0, int64_t b1, void *d) {
    return column_major ? js.rect(m + b0, m + b1, 0, m, DA_OUT_F64, d, cols, nullptr) : js.rect(b0, b1, m, m + n, DA_OUT_F64, d, cols, nullptr);
  });
}

int da_similarity_jaccard_cross_topk_long(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues,
                                          const int64_t *y_offsets, int64_t n, int k, int top, int32_t *idx_out, double *val_out) {
  if (k <= 0) return fail(DA_ERR_BAD_K, "%s", da_status_message(DA_ERR_BAD_K));
  if (m <= 0) return DA_OK;                              // no rows: nothing to write
  if (n <= 0) return fail(DA_ERR_BAD_ARG, "top must be in 1 .. n (got top = %d, n = 0)", top);
  JaccardSets js(1024);
  int rc;
  if ((rc = js.check_two(x_residues, x_offsets, m, y_residues, y_offsets, n, k, idx_out != nullptr)) != DA_OK || (rc = topk_check(top, n)) != DA_OK ||
      (rc = js.build(x_residues, x_offsets, y_residues, y_offsets)) != DA_OK) return rc;
  RankBlocks keys(m, n, false, js.shingles(), [&](int64_t b0, int64_t b1, int64_t, void *d, int64_t ld, bool) {
    return js.rect(b0, b1, m, m + n, DA_OUT_PACK32, d, ld, nullptr);
  }, nullptr);
  return rank_topk_to_host(keys, m, top, false, idx_out, val_out, nullptr);
}

int da_similarity_jaccard_knn_long(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, int top, int32_t *idx_out, double *val_out) {
  JaccardSets js(1024);
  int rc;
  if ((rc = js.check_one(residues, offsets, n, k, idx_out != nullptr)) != DA_OK || (rc = knn_check(top, n)) != DA_OK ||
      (rc = js.build(residues, offsets)) != DA_OK) return rc;
  // not `square`: a block holds all n columns of its rows; the block that is the whole square is computed by the symmetric form
  RankBlocks keys(n, n, false, js.shingles(), [&](int64_t b0, int64_t b1, int64_t, void *d, int64_t ld, bool) {
    return js.rect(b0, b1, 0, n, DA_OUT_PACK32, d, ld, nullptr);
  }, nullptr);
  return rank_topk_to_host(keys, n, top, true, idx_out, val_out, nullptr);
}

int da_similarity_jaccard_edges_long_begin(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, double thresh_p, da_edges **handle_out,
                                           double *threshold_out, int64_t *n_edges_out) {
  return edges_run_handle(handle_out, threshold_out, n_edges_out, [&](bool, EdgeSet &es, int64_t *n_edges) -> int {
    JaccardSets js(1024);
    int rc;
    if ((rc = js.check_one(residues, offsets, n, k, true)) != DA_OK) return rc;
    if (n < 2) return fail(DA_ERR_BAD_ARG, "the threshold is a quantile of the strict upper triangle: need >= 2 sequences");
    if (!(thresh_p >= 0.0 && thresh_p <= 1.0)) return fail(DA_ERR_BAD_ARG, "thresh_p must be in [0, 1]");
    if ((rc = js.build(residues, offsets)) != DA_OK) return rc;
    // rows [b0, b1) against columns [c0 = b0, n); the whole square (b0 = 0, b1 = n) is the symmetric form
    RankKeys keys(n, n, true, js.shingles(), [&](int64_t b0, int64_t b1, int64_t c0, void *d, int64_t ld, bool) {
      return js.rect(b0, b1, c0, n, DA_OUT_PACK32, d, ld, nullptr);
    }, nullptr);
    return edges_to_host(keys, n, thresh_p, true, es, n_edges);
  });
}

int da_similarity_jaccard_cross_edges_long_begin(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues,
                                                 const int64_t *y_offsets, int64_t n, int k, double thresh, int thresh_is_quantile,
                                                 da_edges **handle_out, double *threshold_out, int64_t *n_edges_out) {
  return edges_run_handle(handle_out, threshold_out, n_edges_out, [&](bool, EdgeSet &es, int64_t *n_edges) -> int {
    if (k <= 0) return fail(DA_ERR_BAD_K, "%s", da_status_message(DA_ERR_BAD_K));
    int rc;
    if (m <= 0 || n <= 0) {                                // an empty rectangle: no edges; it has no quantile
      if ((rc = thresh_arg_check(thresh, thresh_is_quantile)) != DA_OK) return rc;
      if (thresh_is_quantile) return fail(DA_ERR_BAD_ARG, "quantile of an empty set");
      es.threshold = thresh;
      *n_edges = 0;
      return DA_OK;
    }
    JaccardSets js(1024);
    if ((rc = js.check_two(x_residues, x_offsets, m, y_residues, y_offsets, n, k, true)) != DA_OK ||
        (rc = thresh_arg_check(thresh, thresh_is_quantile)) != DA_OK || (rc = js.build(x_residues, x_offsets, y_residues, y_offsets)) != DA_OK) return rc;
    RankKeys keys(m, n, false, js.shingles(), [&](int64_t b0, int64_t b1, int64_t, void *d, int64_t ld, bool) {
      return js.rect(b0, b1, m, m + n, DA_OUT_PACK32, d, ld, nullptr);
    }, nullptr);
    return edges_to_host(keys, m, thresh, thresh_is_quantile != 0, es, n_edges);
  });
}

// rank_stats on the rectangle kernel.  Empty sets are legal (J = 1.0 for two of them, 0.0 against a non-empty one): no sequence is refused for
// being empty, unlike in the NW calls.
int da_similarity_jaccard_stats_long(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, da_similarity_stats *out) {
  JaccardSets js(1024);
  int rc;
  if ((rc = js.check_one(residues, offsets, n, k, out != nullptr)) != DA_OK) return rc;
  if (n < 2) return fail(DA_ERR_BAD_ARG, "the statistics are over the strict upper triangle: need >= 2 sequences");
  if ((rc = js.build(residues, offsets)) != DA_OK) return rc;
  RankBlocks keys(n, n, true, js.shingles(), [&](int64_t b0, int64_t b1, int64_t c0, void *d, int64_t ld, bool) {
    return js.rect(b0, b1, c0, n, DA_OUT_PACK32, d, ld, nullptr);
  }, nullptr);
  return rank_stats(keys, n, out);
}

// ---- the Levenshtein similarity on the host boundary (dynaalign.h; lev_kernels.hip) --------------------------------------------------------------
// The operand of every host call, the sibling of JaccardSets without k.  check_one / check_two: the documented validation of one set / of x
// then y, before a device is needed.  build(): DA_ERR_NO_DEVICE last, then one pass over the bytes for the class map, the sequences -- two
// sets as ONE operand [x ; y] of m + n sequences -- and their match masks (k_lev_masks) on the device.  rect(): rows x columns of that operand
// as uint16 codes ((L - d) << 8 | L) or doubles.  The codes have the NW code's shape with L <= 127: every tail of the short Jaccard calls
// applies with the same value table and the same rank table.
struct LevMasks {
  int64_t m = 0, n = 0;                                  // one set: m == 0, n sequences; two sets: x has m, y has n
  int64_t x_total = 0, y_total = 0, max_len = 0;
  int n_classes = 1;
  uint8_t class_map[256];
  DeviceInput in;
  DevBuf masks;
  static int lengths(const int64_t *off, int64_t cnt) {
    for (int64_t i = 0; i < cnt; ++i) {
      const int rc = off[i + 1] - off[i] > 127 ? lev_limits(off[i + 1] - off[i], i + 1) : DA_OK;
      if (rc != DA_OK) return rc;
    }
    return DA_OK;
  }
  int check_one(const uint8_t *res, const int64_t *off, int64_t n_, bool out_ok) {
    if (n_ <= 0) return fail(DA_ERR_EMPTY_INPUT, "%s", da_status_message(DA_ERR_EMPTY_INPUT));
    if (!res || !out_ok) return fail(DA_ERR_BAD_ARG, "NULL pointer");
    int rc;
    if ((rc = check_offsets(off, n_, &y_total, &max_len)) != DA_OK || (rc = lengths(off, n_)) != DA_OK) return rc;
    if (n_ > 0x7ffffff0LL) return fail(DA_ERR_UNSUPPORTED, "Levenshtein: too many sequences");
    m = 0; n = n_;
    return DA_OK;
  }
  // (the empty shapes are the caller's: they differ between the two-set calls)
  int check_two(const uint8_t *xr, const int64_t *xo, int64_t m_, const uint8_t *yr, const int64_t *yo, int64_t n_, bool out_ok) {
    if (!xr || !yr || !out_ok) return fail(DA_ERR_BAD_ARG, "NULL pointer");
    int64_t x_max, y_max;
    int rc;
    if ((rc = check_offsets(xo, m_, &x_total, &x_max)) != DA_OK || (rc = check_offsets(yo, n_, &y_total, &y_max)) != DA_OK) return rc;
    if ((rc = lengths(xo, m_)) != DA_OK || (rc = lengths(yo, n_)) != DA_OK) return rc;
    if (m_ + n_ > 0x7ffffff0LL) return fail(DA_ERR_UNSUPPORTED, "Levenshtein: too many sequences");
    max_len = std::max(x_max, y_max);
    m = m_; n = n_;
    return DA_OK;
  }
  // the byte values that occur, in ascending order, are the classes 0 .. n_classes - 1 (a call without any byte has the one class 0)
  void classes(const uint8_t *a, int64_t a_bytes, const uint8_t *b, int64_t b_bytes) {
    bool seen[256] = {false};
    for (int64_t p = 0; p < a_bytes; ++p) seen[a[p]] = true;
    for (int64_t p = 0; p < b_bytes; ++p) seen[b[p]] = true;
    int c = 0;
    for (int v = 0; v < 256; ++v) class_map[v] = (uint8_t)(seen[v] ? c++ : 0);
    n_classes = std::max(c, 1);
  }
  int operand() {
    int rc;
    const size_t bytes = lev_masks_bytes(m + n, max_len, n_classes);
    if ((rc = masks.alloc(bytes)) != DA_OK) return rc;
    return launch_lev_masks(in.res.as<uint8_t>(), in.off.as<int64_t>(), m + n, max_len, class_map, n_classes, masks.p, bytes, nullptr);
  }
  int build(const uint8_t *res, const int64_t *off) {
    int rc;
    if ((rc = require_device()) != DA_OK) return rc;
    classes(res, y_total, nullptr, 0);
    if ((rc = in.upload(res, off, n, y_total, nullptr, 0)) != DA_OK) return rc;
    return operand();
  }
  int build(const uint8_t *xr, const int64_t *xo, const uint8_t *yr, const int64_t *yo) {
    int rc;
    if ((rc = require_device()) != DA_OK) return rc;
    classes(xr, x_total, yr, y_total);
    std::vector<uint8_t> res((size_t)(x_total + y_total) + 1);
    std::vector<int64_t> off((size_t)(m + n) + 1);
    if (x_total) memcpy(res.data(), xr, (size_t)x_total);
    if (y_total) memcpy(res.data() + x_total, yr, (size_t)y_total);
    for (int64_t i = 0; i <= m; ++i) off[(size_t)i] = xo[i];
    for (int64_t j = 1; j <= n; ++j) off[(size_t)(m + j)] = x_total + yo[j];
    if ((rc = in.upload(res.data(), off.data(), m + n, x_total + y_total, nullptr, 0)) != DA_OK) return rc;
    return operand();
  }
  int rect(int64_t r0, int64_t r1, int64_t c0, int64_t c1, int kind, void *d, int64_t ld, hipStream_t stream) const {
    return launch_lev_rect(masks.p, m + n, max_len, n_classes, r0, r1, c0, c1, kind, d, ld, stream);
  }
  // the bins the call's uint16 codes fall into: L - d <= L <= max_len (at least 1: the code of two empty strings is 1 << 8 | 1)
  int nbins() const {
    const int64_t len = std::max<int64_t>(1, max_len);
    return (int)((len << 8) | len) + 1;
  }
};

int da_similarity_lev(const uint8_t *residues, const int64_t *offsets, int64_t n, double *out) {
  LevMasks lv;
  int rc;
  if ((rc = lv.check_one(residues, offsets, n, out != nullptr)) != DA_OK || (rc = lv.build(residues, offsets)) != DA_OK) return rc;
  Trace tr("similarityLev host path");
  const std::vector<double> table = nw_code_values(65536, 0.0);
  if (rows_per_block(n, sizeof(uint16_t)) >= n)
    return codes_to_host(n, out, table, tr, [&](void *d) { return lv.rect(0, n, 0, n, DA_OUT_COMPACT, d, n, nullptr); });
  return rows_to_host(n, 0, n, sizeof(uint16_t), out, [&](int64_t b0, int64_t b1, void *d) { return lv.rect(b0, b1, 0, n, DA_OUT_COMPACT, d, n, nullptr); },
                      nullptr, nullptr, table.data());
}

int da_similarity_lev_cross(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues, const int64_t *y_offsets,
                            int64_t n, double *out, int column_major) {
  if (m <= 0 || n <= 0) return DA_OK;                    // an m x 0 or 0 x n matrix: nothing to write
  LevMasks lv;
  int rc;
  if ((rc = lv.check_two(x_residues, x_offsets, m, y_residues, y_offsets, n, out != nullptr)) != DA_OK ||
      (rc = lv.build(x_residues, x_offsets, y_residues, y_offsets)) != DA_OK) return rc;
  const int64_t rows = column_major ? n : m, cols = column_major ? m : n;
  const std::vector<double> table = nw_code_values(65536, 0.0);
  // the distance is symmetric: rows of y against columns of x are the transpose, R's column-major NumericMatrix(m, n)
  return rows_to_host(cols, 0, rows, sizeof(uint16_t), out, [&](int64_t b0, int64_t b1, void *d) {
    return column_major ? lv.rect(m + b0, m + b1, 0, m, DA_OUT_COMPACT, d, cols, nullptr) : lv.rect(b0, b1, m, m + n, DA_OUT_COMPACT, d, cols, nullptr);
  }, nullptr, nullptr, table.data());
}

int da_similarity_lev_cross_topk(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues, const int64_t *y_offsets,
                                 int64_t n, int top, int32_t *idx_out, double *val_out) {
  if (m <= 0) return DA_OK;                              // no rows: nothing to write
  if (n <= 0) return fail(DA_ERR_BAD_ARG, "top must be in 1 .. n (got top = %d, n = 0)", top);
  LevMasks lv;
  int rc, bits = 16;
  if ((rc = lv.check_two(x_residues, x_offsets, m, y_residues, y_offsets, n, idx_out != nullptr)) != DA_OK || (rc = topk_check(top, n)) != DA_OK ||
      (rc = lv.build(x_residues, x_offsets, y_residues, y_offsets)) != DA_OK) return rc;
  DevBuf drank, didx, dkey;
  if ((rc = jaccard_ranks(drank, &bits)) != DA_OK || (rc = didx.alloc((size_t)m * (size_t)top * sizeof(int32_t))) != DA_OK ||
      (rc = dkey.alloc((size_t)m * (size_t)top * sizeof(uint16_t))) != DA_OK) return rc;
  rc = topk_blocks(m, n, drank.as<uint16_t>(), bits, top, didx.as<int32_t>(), top, dkey.as<uint16_t>(), top, nullptr,
                   [&](int64_t b0, int64_t b1, void *d, int64_t ld) { return lv.rect(b0, b1, m, m + n, DA_OUT_COMPACT, d, ld, nullptr); });
  if (rc != DA_OK) return rc;
  return topk_to_host(didx, dkey, m, top, nw_code_values(65536, 0.0), idx_out, val_out);
}

int da_similarity_lev_knn(const uint8_t *residues, const int64_t *offsets, int64_t n, int top, int32_t *idx_out, double *val_out) {
  LevMasks lv;
  int rc, bits = 16;
  if ((rc = lv.check_one(residues, offsets, n, idx_out != nullptr)) != DA_OK || (rc = knn_check(top, n)) != DA_OK ||
      (rc = lv.build(residues, offsets)) != DA_OK) return rc;
  DevBuf drank, didx, dkey;
  if ((rc = jaccard_ranks(drank, &bits)) != DA_OK || (rc = didx.alloc((size_t)n * (size_t)top * sizeof(int32_t))) != DA_OK ||
      (rc = dkey.alloc((size_t)n * (size_t)top * sizeof(uint16_t))) != DA_OK) return rc;
  rc = topk_blocks(n, n, drank.as<uint16_t>(), bits, top, didx.as<int32_t>(), top, dkey.as<uint16_t>(), top, nullptr,
                   [&](int64_t b0, int64_t b1, void *d, int64_t ld) { return lv.rect(b0, b1, 0, n, DA_OUT_COMPACT, d, ld, nullptr); }, true);
  if (rc != DA_OK) return rc;
  return topk_to_host(didx, dkey, n, top, nw_code_values(65536, 0.0), idx_out, val_out);
}

// the similarity + clusterbreak's threshold step as an edge list: the histogram / quantile / extraction path of the NW codes, as
// jaccard_edges_core
static int lev_edges_core(const uint8_t *residues, const int64_t *offsets, int64_t n, double thresh_p, bool want_edges, EdgeSet &es, int64_t *n_edges_out) {
  LevMasks lv;
  int rc;
  if ((rc = lv.check_one(residues, offsets, n, true)) != DA_OK) return rc;
  if (n < 2) return fail(DA_ERR_BAD_ARG, "the threshold is a quantile of the strict upper triangle: need >= 2 sequences");
  if (!(thresh_p >= 0.0 && thresh_p <= 1.0)) return fail(DA_ERR_BAD_ARG, "thresh_p must be in [0, 1]");
  if ((rc = lv.build(residues, offsets)) != DA_OK) return rc;
  DevBuf cnt, hist;
  const int nbins = lv.nbins();
  if ((rc = cnt.alloc((size_t)n * (size_t)n * 2)) != DA_OK || (rc = hist.alloc((size_t)nbins * 8)) != DA_OK) return rc;   // uint16 codes stay on the device
  DA_HIP_TRY(hipMemset(hist.p, 0, (size_t)nbins * 8));
  if ((rc = lv.rect(0, n, 0, n, DA_OUT_COMPACT, cnt.p, n, nullptr)) != DA_OK) return rc;
  if ((rc = launch_upper_histogram(cnt.as<uint16_t>(), n, n, nbins, hist.as<unsigned long long>(), nullptr)) != DA_OK) return rc;
  return edges_from_counts(cnt.as<uint16_t>(), n, nbins, hist.as<unsigned long long>(), nw_code_values(nbins, 0.0), thresh_p, want_edges, es, n_edges_out);
}

int da_similarity_lev_edges(const uint8_t *residues, const int64_t *offsets, int64_t n, double thresh_p, double *threshold_out, int64_t *n_edges_out,
                            int64_t capacity, int32_t *ei, int32_t *ej, double *ew) {
  return edges_run_deliver(threshold_out, n_edges_out, capacity, ei, ej, ew, [&](bool want_edges, EdgeSet &es, int64_t *cnt) {
    return lev_edges_core(residues, offsets, n, thresh_p, want_edges, es, cnt);
  });
}

int da_similarity_lev_edges_begin(const uint8_t *residues, const int64_t *offsets, int64_t n, double thresh_p, da_edges **handle_out,
                                  double *threshold_out, int64_t *n_edges_out) {
  return edges_run_handle(handle_out, threshold_out, n_edges_out, [&](bool want_edges, EdgeSet &es, int64_t *cnt) {
    return lev_edges_core(residues, offsets, n, thresh_p, want_edges, es, cnt);
  });
}

// the range query: every (i, j) of x against y at or above a threshold, as da_similarity_nw_cross_edges_begin
int da_similarity_lev_cross_edges_begin(const uint8_t *x_residues, const int64_t *x_offsets, int64_t m, const uint8_t *y_residues,
                                        const int64_t *y_offsets, int64_t n, double thresh, int thresh_is_quantile, da_edges **handle_out,
                                        double *threshold_out, int64_t *n_edges_out) {
  return edges_run_handle(handle_out, threshold_out, n_edges_out, [&](bool, EdgeSet &es, int64_t *n_edges) -> int {
    int rc;
    if (m <= 0 || n <= 0) {                                // an empty rectangle: no edges; it has no quantile
      if ((rc = thresh_arg_check(thresh, thresh_is_quantile)) != DA_OK) return rc;
      if (thresh_is_quantile) return fail(DA_ERR_BAD_ARG, "quantile of an empty set");
      es.threshold = thresh;
      *n_edges = 0;
      return DA_OK;
    }
    LevMasks lv;
    if ((rc = lv.check_two(x_residues, x_offsets, m, y_residues, y_offsets, n, true)) != DA_OK ||
        (rc = thresh_arg_check(thresh, thresh_is_quantile)) != DA_OK || (rc = lv.build(x_residues, x_offsets, y_residues, y_offsets)) != DA_OK) return rc;
    const std::vector<double> values = nw_code_values(lv.nbins(), 0.0);
    CodeKeys keys(m, n, values, [&](int64_t b0, int64_t b1, void *d, int64_t ld) { return lv.rect(b0, b1, m, m + n, DA_OUT_COMPACT, d, ld, nullptr); }, nullptr);
    return edges_to_host(keys, m, thresh, thresh_is_quantile != 0, es, n_edges);
  });
}


// ------------------------------------------------- multi-device host entry points (SURVEY 8(b) da_opts, 8(e))
// ONE process drives several GPUs: a host thread per device (hipSetDevice is per thread), every device holds all
// sequences and rebuilds all signatures itself (2 MB in), the pair space is split, and every device copies ITS
// rows of the result straight into the caller's matrix -- P PCIe links instead of one, which is where more GPUs help
// the host-pointer boundary (the 80 GB result is PCIe-bound).  Exchange modes:
//   DA_EXCHANGE_ROWS      no device-to-device traffic: device p computes the contiguous row block it will copy out
//                         (full rows: twice the triangle's compare work, still far below the copy time);
//   DA_EXCHANGE_ALLGATHER the north-star's shape: cyclic upper-triangle shards -> ONE ncclAllGather over xGMI (RCCL,
//                         communicators from ncclCommInitAll) -> mirror + widen to the full matrix on every device;
//   DA_EXCHANGE_PEERCOPY  the same shards exchanged by direct hipMemcpyPeerAsync reads of every peer's block: xGMI is
//                         point-to-point, so P - 1 concurrent peer copies use all links at once where a ring is
//                         per-link bound; needs no RCCL.
// RCCL is bound at run time (dlopen of librccl.so.1): a process that already carries an RCCL (PyTorch's) keeps one copy.
}  // extern "C"  (reopened below)

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <array>
#include <chrono>

namespace da {
namespace {

struct Rccl {
  void *h = nullptr;
  ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;              // optional: tears down a communicator whose collective may be stuck
  ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
  std::string why;
  bool load() {
    if (h) return true;
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (h) break;
      why = dlerror();
    }
    if (!h) return false;
    CommInitAll = reinterpret_cast<decltype(CommInitAll)>(dlsym(h, "ncclCommInitAll"));
    CommDestroy = reinterpret_cast<decltype(CommDestroy)>(dlsym(h, "ncclCommDestroy"));
    CommAbort = reinterpret_cast<decltype(CommAbort)>(dlsym(h, "ncclCommAbort"));
    AllGather = reinterpret_cast<decltype(AllGather)>(dlsym(h, "ncclAllGather"));
    GetErrorString = reinterpret_cast<decltype(GetErrorString)>(dlsym(h, "ncclGetErrorString"));
    if (!CommInitAll || !CommDestroy || !AllGather || !GetErrorString) { why = "librccl lacks ncclCommInitAll / ncclAllGather"; h = nullptr; return false; }
    return true;
  }
};
Rccl &rccl() { static Rccl r; return r; }
std::mutex &rccl_mutex() { static std::mutex m; return m; }

// all ranks arrive with their status; everyone learns whether all were fine
class StatusBarrier {
 public:
  explicit StatusBarrier(int n) : n_(n) {}
  bool arrive(bool ok) {
    std::unique_lock<std::mutex> g(m_);
    if (!ok) all_ok_ = false;
    const uint64_t gen = gen_;
    if (++count_ == n_) { count_ = 0; result_ = all_ok_; ++gen_; cv_.notify_all(); return result_; }
    cv_.wait(g, [&]() { return gen_ != gen; });
    return result_;
  }
 private:
  std::mutex m_;
  std::condition_variable cv_;
  int n_, count_ = 0;
  uint64_t gen_ = 0;
  bool all_ok_ = true, result_ = true;
};

enum { PH_SETUP = 0, PH_COMPUTE, PH_EXCHANGE, PH_FINALIZE, PH_D2H, PH_TOTAL, PH_COUNT };

struct Multi {
  int P = 1, exchange = DA_EXCHANGE_ROWS;
  std::vector<int> devs;
  std::vector<ncclComm_t> comms;
  std::vector<const void *> block;                 // rank p's block to exchange (device pointer), PEERCOPY
  std::vector<int> rc;
  std::vector<std::string> msg;
  std::vector<std::array<double, PH_COUNT>> ms;
  std::unique_ptr<StatusBarrier> bar;
  double t_entry = 0.0, comm_setup_ms = 0.0;       // entry of the C call; ncclCommInitAll (first call with this device list)
  std::unique_lock<std::mutex> comm_use;           // held while this call uses the cached communicators
};

// RCCL communicators are kept per device list: ncclCommInitAll costs far more than the exchange it serves, and the glue calls
// once per recursion level.  One call at a time uses them (comm_use_mutex); da_release_device_memory() destroys them.
std::map<std::vector<int>, std::vector<ncclComm_t>> &comm_cache() { static auto *c = new std::map<std::vector<int>, std::vector<ncclComm_t>>; return *c; }
std::mutex &comm_use_mutex() { static std::mutex m; return m; }

// rows rank p copies to the host: contiguous, boundaries on 128-row tiles
void row_split(int64_t n, int P, int p, int64_t *r0, int64_t *r1) {
  const int64_t T = ceil_div(n, 128);
  *r0 = std::min(n, ceil_div(T * p, P) * 128);
  *r1 = std::min(n, ceil_div(T * (p + 1), P) * 128);
}

int parse_opts(const da_opts *o, Multi &m) {
  m.t_entry = now_ms();                              // phase_ms[5] is the whole call: validation and communicator setup included
  m.P = 1; m.exchange = DA_EXCHANGE_ROWS; m.devs.clear();
  if (o) {
    if (o->struct_size < (uint32_t)offsetof(da_opts, phase_ms)) return fail(DA_ERR_BAD_ARG, "da_opts.struct_size is not set (sizeof(da_opts))");
    if (o->n_devices < 0 || (o->n_devices > 0 && !o->devices)) return fail(DA_ERR_BAD_ARG, "bad device list");
    if (o->exchange != DA_EXCHANGE_ROWS && o->exchange != DA_EXCHANGE_ALLGATHER && o->exchange != DA_EXCHANGE_PEERCOPY)
      return fail(DA_ERR_BAD_ARG, "unknown exchange mode %d", o->exchange);
    m.exchange = o->exchange;
    for (int i = 0; i < o->n_devices; ++i) m.devs.push_back(o->devices[i]);
  }
  int rc = require_device();
  if (rc != DA_OK) return rc;
  int cnt = 0;
  DA_HIP_TRY(hipGetDeviceCount(&cnt));
  if (m.devs.empty()) { int cur = 0; DA_HIP_TRY(hipGetDevice(&cur)); m.devs.push_back(cur); }
  for (size_t i = 0; i < m.devs.size(); ++i) {
    if (m.devs[i] < 0 || m.devs[i] >= cnt) return fail(DA_ERR_BAD_ARG, "device %d not present (%d visible)", m.devs[i], cnt);
    if (m.exchange == DA_EXCHANGE_ALLGATHER)          // RCCL refuses two ranks on one GPU; the other modes allow it (tests on a 1-GPU box)
      for (size_t j = 0; j < i; ++j)
        if (m.devs[j] == m.devs[i]) return fail(DA_ERR_BAD_ARG, "device %d listed twice (not allowed with DA_EXCHANGE_ALLGATHER)", m.devs[i]);
  }
  m.P = (int)m.devs.size();
  m.rc.assign(m.P, DA_OK); m.msg.assign(m.P, ""); m.block.assign(m.P, nullptr);
  m.ms.assign(m.P, std::array<double, PH_COUNT>{});
  m.bar.reset(new StatusBarrier(m.P));
  if (m.exchange == DA_EXCHANGE_ALLGATHER) {
    m.comm_use = std::unique_lock<std::mutex>(comm_use_mutex());
    std::lock_guard<std::mutex> g(rccl_mutex());
    if (!rccl().load()) { m.comm_use.unlock(); return fail(DA_ERR_UNSUPPORTED, "DA_EXCHANGE_ALLGATHER needs RCCL: %s", rccl().why.c_str()); }
    auto it = comm_cache().find(m.devs);
    if (it == comm_cache().end()) {
      const double t0 = now_ms();
      std::vector<ncclComm_t> comms((size_t)m.P, nullptr);
      const ncclResult_t r = rccl().CommInitAll(comms.data(), m.P, m.devs.data());
      if (r != ncclSuccess) { m.comm_use.unlock(); return fail(DA_ERR_HIP, "ncclCommInitAll failed: %s", rccl().GetErrorString(r)); }
      m.comm_setup_ms = now_ms() - t0;
      it = comm_cache().emplace(m.devs, std::move(comms)).first;
    }
    m.comms = it->second;
  }
  return DA_OK;
}

// the communicators stay cached (destroy_cached_comms); the call only gives up its right to use them.  `failed`: some rank of this
// call returned an error -- a communicator that has seen a failed or abandoned collective may hang the next one, so the cache entry of
// this device list is torn down (ncclCommAbort where the library has it) before the lock is released; the next call makes new ones.
size_t g_comm_evictions = 0;                        // (tests: da_debug_comm_cache_state)
void destroy_comms(Multi &m, bool failed = false) {
  if (failed && m.exchange == DA_EXCHANGE_ALLGATHER && m.comm_use.owns_lock()) {
    std::lock_guard<std::mutex> g(rccl_mutex());
    auto it = comm_cache().find(m.devs);
    if (it != comm_cache().end()) {
      for (auto c : it->second)
        if (c) (void)(rccl().CommAbort ? rccl().CommAbort(c) : rccl().CommDestroy(c));
      comm_cache().erase(it);
      ++g_comm_evictions;
    }
  }
  m.comms.clear();
  if (m.comm_use.owns_lock()) m.comm_use.unlock();
}

// direct xGMI reads of the peers' blocks (PEERCOPY); without it hipMemcpyPeer stages through the host
void enable_peer_access(const Multi &m, int p) {
  for (int q = 0; q < m.P; ++q)
    if (m.devs[q] != m.devs[p]) {
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, m.devs[p], m.devs[q]) == hipSuccess && can) {
        const hipError_t e = hipDeviceEnablePeerAccess(m.devs[q], 0);
        if (e != hipSuccess) (void)hipGetLastError();   // already enabled: fine
      }
    }
}

// run body(p) on one host thread per rank; the first failing rank's status / message become the caller's
template <typename F> int run_ranks(Multi &m, const da_opts *o, F body) {
  const double t0 = m.t_entry > 0.0 ? m.t_entry : now_ms();
  auto one = [&](int p) {
    int rc = DA_OK;
    if (hipSetDevice(m.devs[p]) != hipSuccess) rc = fail(DA_ERR_HIP, "hipSetDevice(%d) failed", m.devs[p]);
    if (rc == DA_OK && m.exchange == DA_EXCHANGE_PEERCOPY) enable_peer_access(m, p);
    if (rc == DA_OK) rc = body(p);
    m.rc[p] = rc;
    if (rc != DA_OK) m.msg[p] = last_error_ref();
  };
  int cur = 0;
  (void)hipGetDevice(&cur);
  if (m.P == 1) one(0);
  else {
    std::vector<std::thread> th;
    for (int p = 0; p < m.P; ++p) th.emplace_back(one, p);
    for (auto &t : th) t.join();
  }
  (void)hipSetDevice(cur);
  bool any_failed = false;
  for (int p = 0; p < m.P; ++p) any_failed = any_failed || m.rc[p] != DA_OK;
  destroy_comms(m, any_failed);
  if (o && o->struct_size >= sizeof(da_opts) && o->phase_ms) {
    for (int k = 0; k < PH_COUNT; ++k) {
      double mx = 0.0;
      for (int p = 0; p < m.P; ++p) mx = std::max(mx, m.ms[p][k]);
      o->phase_ms[k] = mx;
    }
    o->phase_ms[PH_SETUP] += m.comm_setup_ms;          // ncclCommInitAll, paid by the first call with this device list
    o->phase_ms[PH_TOTAL] = now_ms() - t0;
  }
  for (int p = 0; p < m.P; ++p)
    if (m.rc[p] != DA_OK) { last_error_ref() = m.msg[p]; return m.rc[p]; }
  return DA_OK;
}

// the exchange step of the sharded modes: my block (bytes) -> gathered[P][bytes] on this rank's device
int exchange_blocks(Multi &m, int p, const void *mine, size_t bytes, void *gathered) {
  if (m.exchange == DA_EXCHANGE_ALLGATHER) {
    const ncclResult_t r = rccl().AllGather(mine, gathered, bytes, ncclUint8, m.comms[p], nullptr);
    if (r != ncclSuccess) return fail(DA_ERR_HIP, "ncclAllGather failed: %s", rccl().GetErrorString(r));
    DA_HIP_TRY(hipStreamSynchronize(nullptr));
    return DA_OK;
  }
  // PEERCOPY: every peer's block is complete (the barrier before this call); read them all, concurrently
  for (int q = 0; q < m.P; ++q) {
    char *dst = static_cast<char *>(gathered) + (size_t)q * bytes;
    if (m.devs[q] == m.devs[p]) DA_HIP_TRY(hipMemcpyAsync(dst, m.block[q], bytes, hipMemcpyDeviceToDevice, nullptr));
    else DA_HIP_TRY(hipMemcpyPeerAsync(dst, m.devs[p], m.block[q], m.devs[q], bytes, nullptr));
  }
  DA_HIP_TRY(hipStreamSynchronize(nullptr));
  return DA_OK;
}

// da_debug_comm_cache_state(force_fail != 0): rank 0 of the next DA_EXCHANGE_ALLGATHER call fails right after its compute phase
std::atomic<int> g_force_exchange_error{0};

// Rank p of a sharded mode (ALLGATHER, PEERCOPY) after its setup, which returned rc: compute(local, block) fills this rank's cyclic
// upper-triangle tiles into local (sg.rows x sg.W uint16, zeroed) and leaves the block to exchange in `block` -- a buffer of
// pack_bytes, or local itself when pack_bytes is 0; after the exchange, finalize(gathered, dout) builds the full n x n float64 matrix
// from every rank's block, and this rank copies its rows of it to out.  A rank whose setup or compute failed still arrives at the
// first barrier: every rank then learns of the failure there and returns.
template <typename Compute, typename Finalize>
int sharded_rank(Multi &m, int p, int rc, int64_t n, const ShardGeom &sg, size_t pack_bytes, double *out, Compute compute,
                 Finalize finalize) {
  const size_t local_bytes = (size_t)sg.rows * (size_t)sg.W * 2, bytes = pack_bytes ? pack_bytes : local_bytes;
  DevBuf local, pk, gathered, dout;
  int64_t r0, r1;
  row_split(n, m.P, p, &r0, &r1);
  double t = now_ms();
  if (rc == DA_OK) do {
    if ((rc = local.alloc(local_bytes)) != DA_OK) break;
    if (pack_bytes && (rc = pk.alloc(pack_bytes)) != DA_OK) break;
    if ((rc = gathered.alloc(bytes * (size_t)m.P)) != DA_OK) break;
    if ((rc = dout.alloc((size_t)n * (size_t)n * sizeof(double))) != DA_OK) break;
    if (hipMemsetAsync(local.p, 0, local_bytes, nullptr) != hipSuccess) { rc = fail(DA_ERR_HIP, "hipMemsetAsync failed"); break; }
    rc = compute(local.p, pack_bytes ? pk.p : local.p);
  } while (0);
  m.ms[p][PH_COMPUTE] = now_ms() - t;
  m.block[p] = pack_bytes ? pk.p : local.p;
  if (p == 0 && rc == DA_OK && m.exchange == DA_EXCHANGE_ALLGATHER && g_force_exchange_error.exchange(0))   // (test hook)
    rc = fail(DA_ERR_HIP, "forced exchange failure (test hook)");
  if (!m.bar->arrive(rc == DA_OK)) return rc;     // every block is complete (and nobody failed) before anyone exchanges
  t = now_ms();
  rc = exchange_blocks(m, p, m.block[p], bytes, gathered.p);
  m.ms[p][PH_EXCHANGE] = now_ms() - t;
  if (!m.bar->arrive(rc == DA_OK)) return rc;     // peers have finished reading my block before it is freed
  t = now_ms();
  if ((rc = finalize(gathered.p, dout.as<double>())) != DA_OK) return rc;
  if ((rc = sync_or_fail("finalize kernel failed")) != DA_OK) return rc;
  m.ms[p][PH_FINALIZE] = now_ms() - t;
  t = now_ms();
  if (r1 > r0) rc = d2h_pipelined(out + (size_t)r0 * (size_t)n, dout.as<double>() + (size_t)r0 * (size_t)n, (size_t)(r1 - r0) * (size_t)n * sizeof(double));
  m.ms[p][PH_D2H] = now_ms() - t;
  return rc;
}

}  // namespace

size_t destroy_cached_comms() {
  std::lock_guard<std::mutex> u(comm_use_mutex());
  std::lock_guard<std::mutex> g(rccl_mutex());
  size_t k = 0;
  for (auto &e : comm_cache())
    for (auto c : e.second) if (c) { (void)rccl().CommDestroy(c); ++k; }
  comm_cache().clear();
  return k;
}
}  // namespace da

extern "C" {

/* tests: {cached device lists, evictions after a failed ALLGATHER call}; with force_fail != 0 the NEXT DA_EXCHANGE_ALLGATHER call's rank 0
 * (similarityMH or similarityNW) fails right after its compute phase (before the collective) -- every rank then skips the exchange and
 * the cache entry must go */
int da_debug_comm_cache_state(int force_fail, size_t *out2) {
  std::lock_guard<std::mutex> u(da::comm_use_mutex());
  if (out2) { out2[0] = da::comm_cache().size(); out2[1] = da::g_comm_evictions; }
  if (force_fail) g_force_exchange_error.store(1);
  return DA_OK;
}

int da_rccl_available(void) {
  std::lock_guard<std::mutex> g(rccl_mutex());
  return rccl().load() ? 1 : 0;
}

int da_similarity_mh_opts(const uint8_t *residues, const int64_t *offsets, int64_t n, int k, int n_hash,
                          const uint32_t *seeds, double *out, const da_opts *opts) {
  int rc = validate_mh(n, k, n_hash);
  if (rc != DA_OK) return rc;
  if (!residues || !seeds || !out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  int64_t total, max_len;
  if ((rc = check_offsets(offsets, n, &total, &max_len)) != DA_OK) return rc;
  Multi m;
  if ((rc = parse_opts(opts, m)) != DA_OK) return rc;
  if (n_hash > 65535 && !(m.P == 1 && m.exchange == DA_EXCHANGE_ROWS)) {
    destroy_comms(m);
    return fail(DA_ERR_UNSUPPORTED, "n_hash = %d (> 65535) runs on one device only (16-bit counters in the sharded kernels)", n_hash);
  }
  if (m.P == 1 && m.exchange == DA_EXCHANGE_ROWS)      // one device, nothing to split: the symmetric single-device path
    return run_ranks(m, opts, [&](int) -> int {
      return mh_host_common(residues, offsets, n, k, n_hash, seeds, 0, n, DA_OUT_F64, out);
    });
  const int vbits = std::max(8, 32 - __builtin_clz((unsigned)n_hash));
  const ShardGeom sg = shard_geom(n, m.P, 128);
  const size_t packed = (size_t)shard_packed_bytes(sg, vbits);
  return run_ranks(m, opts, [&](int p) -> int {
    const double t = now_ms();
    MhPlanes mh;
    int rc;
    do {   // setup: upload + K1 + K1b on this device
      if ((rc = mh.in.upload(residues, offsets, n, total, seeds, n_hash)) != DA_OK) break;
      if ((rc = mh.alloc(n, n_hash)) != DA_OK || (rc = mh.build(k, 0, n_hash)) != DA_OK) break;
      if (mh.finish() != DA_OK) rc = fail(DA_ERR_HIP, "stream synchronisation failed");
    } while (0);
    m.ms[p][PH_SETUP] = now_ms() - t;
    if (m.exchange != DA_EXCHANGE_ROWS)   // cyclic upper-triangle tiles -> packed block -> exchange -> full matrix on this device
      return sharded_rank(m, p, rc, n, sg, packed, out, [&](void *local, void *pk) {
        int rc;
        if ((int64_t)p * 128 < n &&
            (rc = launch_mh_compare(mh.planes.as<uint32_t>(), n, n_hash, (int64_t)p * 128, n, false, DA_OUT_COMPACT, local, sg.W, nullptr,
                                    mh.bits, m.P, true, sg.Q, sg.W)) != DA_OK) return rc;
        if ((rc = launch_pack_shard(static_cast<const uint16_t *>(local), sg.W, sg, vbits, static_cast<uint8_t *>(pk), nullptr)) != DA_OK)
          return rc;
        return sync_or_fail("shard compare failed");
      }, [&](const void *gathered, double *dout) {
        return launch_finalize_packed(static_cast<const uint8_t *>(gathered), sg, vbits, n_hash, dout, n, nullptr);
      });
    int64_t r0, r1;
    row_split(n, m.P, p, &r0, &r1);
    if (rc != DA_OK || r1 <= r0) return rc;
    return rows_to_host(n, r0, r1, sizeof(double), out + (size_t)r0 * (size_t)n, [&](int64_t b0, int64_t b1, void *d) {
      const int rc = launch_mh_compare(mh.planes.as<uint32_t>(), n, n_hash, b0, b1, false, DA_OUT_F64, d, n, nullptr, mh.bits);
      return rc != DA_OK ? rc : sync_or_fail("compare kernel failed");
    }, &m.ms[p][PH_COMPUTE], &m.ms[p][PH_D2H]);
  });
}

int da_similarity_nw_opts(const uint8_t *residues, const int64_t *offsets, int64_t n, const char *matrix_name, int gap_open,
                          int gap_ext, double *out, const da_opts *opts) {
  const int mid = da_matrix_id(matrix_name);          // reference :338 -> :190-206, before anything else
  if (mid < 0) return DA_ERR_BAD_MATRIX;
  if (n <= 0) return DA_OK;                            // reference returns a 0x0 matrix
  if (!residues || !out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  int64_t total, max_len;
  int rc;
  if ((rc = check_offsets(offsets, n, &total, &max_len)) != DA_OK) return rc;
  if ((rc = nw_validate(residues, offsets, n)) != DA_OK) return rc;
  Multi m;
  if ((rc = parse_opts(opts, m)) != DA_OK) return rc;
  if (m.exchange != DA_EXCHANGE_ROWS && max_len > 64) {
    destroy_comms(m);
    return fail(DA_ERR_UNSUPPORTED, "the sharded NW exchange works on uint16 codes of sequences up to 64 residues (longest here: %lld); "
                                    "use DA_EXCHANGE_ROWS", (long long)max_len);
  }
  if (m.P == 1 && m.exchange == DA_EXCHANGE_ROWS)
    return run_ranks(m, opts, [&](int) -> int {
      return nw_host_common(residues, offsets, n, matrix_name, gap_open, gap_ext, 0, n, out, nullptr, nullptr, nullptr);
    });
  const ShardGeom sg = shard_geom(n, m.P, 128);
  return run_ranks(m, opts, [&](int p) -> int {
    const double t = now_ms();
    NwCodes nw;
    int rc = nw.upload(residues, offsets, n, total);
    m.ms[p][PH_SETUP] = now_ms() - t;
    const uint8_t *codes = nw.codes.as<uint8_t>();
    const int64_t *d_off = nw.in.off.as<int64_t>();
    if (m.exchange != DA_EXCHANGE_ROWS)
      return sharded_rank(m, p, rc, n, sg, 0, out, [&](void *local, void *) {
        const int rc = launch_nw(codes, d_off, n, max_len, mid, gap_open, gap_ext, 0, n, false, DA_OUT_COMPACT, local, sg.W, nullptr, 0,
                                 nullptr, p, m.P);
        return rc != DA_OK ? rc : sync_or_fail("NW shard kernel failed");
      }, [&](const void *gathered, double *dout) {
        return launch_finalize_sharded(static_cast<const uint16_t *>(gathered), sg.W, sg, true, 0, dout, n, nullptr);
      });
    int64_t r0, r1;
    row_split(n, m.P, p, &r0, &r1);
    if (rc != DA_OK || r1 <= r0) return rc;
    return rows_to_host(n, r0, r1, sizeof(double), out + (size_t)r0 * (size_t)n, [&](int64_t b0, int64_t b1, void *d) {
      const int rc = launch_nw(codes, d_off, n, max_len, mid, gap_open, gap_ext, b0, b1, false, DA_OUT_F64, d, n, nullptr, 0, nullptr);
      return rc != DA_OK ? rc : sync_or_fail("NW kernel failed");
    }, &m.ms[p][PH_COMPUTE], &m.ms[p][PH_D2H]);
  });
}

}  // extern "C"
