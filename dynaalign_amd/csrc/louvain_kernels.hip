// louvain_kernels.hip -- the synchronous Louvain of clusterbreak.louvain_sync_dense on the device (da_dev_louvain_csr).
//
// The definition is the numpy function; this file reproduces it bit for bit.  What makes that possible:
//   * every weight is the integer rint(w * 2^30) and every sum of weights (strengths k, community totals tot, weight into a community,
//     internal weight IN, coarse edge weights) is an exact 64-bit integer, so no result depends on the order in which lanes, waves or
//     atomics arrive;
//   * the gain of a candidate is ONE fixed expression in doubles, g(w, t) = (double)w - ((res * (double)t) * (double)k_v) / (double)m2,
//     evaluated per candidate with contraction off, and the maximum is taken in the total order (gain descending, id ascending);
//   * a sub-round is two launches: k_lv_decide reads comm / tot / size and writes next[], k_lv_apply then moves the vertices.  There is
//     no grid-wide barrier, no persistent kernel and no float atomic; the host loop is bounded by 32 levels x 64 iterations x 8 classes,
//     and probing in a hash table is bounded by the table size (exhaustion raises an error flag, it does not spin).
//
// Decide kernels by degree (limits in DESIGN.md section 7):
//   bin 0  rows of <= 64 entries: a wave per row, a lane per entry, equal communities combined by comparing against every lane (shuffles);
//   bin 1  rows of <= 3072 entries: a workgroup per row and an open-addressing table (int32 key, int64 value, 4096 slots = 48 KiB) in LDS;
//          on a level of <= 4096 vertices the table is indexed by the community id directly and takes rows of any length;
//   bin 2  longer rows: the LDS table is tried first (a long row has few neighbouring communities once the first sub-rounds have merged
//          them); a row whose communities do not fit takes the same table in the workspace, sized from the level's largest degree, one
//          per workgroup of a bounded pool.
#include "lsh_common.hpp"

#include <climits>
#include <cmath>
#include <vector>

#pragma clang fp contract(off)

namespace da {
namespace {

constexpr int LV_THREADS = 256;
constexpr int LV_WAVES = LV_THREADS / 64;
constexpr int LV_CLASSES = 8, LV_BINS = 3, LV_BUCKETS = LV_CLASSES * LV_BINS;
constexpr int LV_MAX_ITERATIONS = 64, LV_MAX_LEVELS = 32;
constexpr int LV_WAVE_MAX = 64;          // bin 0: one lane per entry
constexpr int LV_LDS_SLOTS = 4096;       // bin 1: 4096 x (4 + 8) B = 48 KiB -> three workgroups share a CU's 160 KiB
constexpr int LV_LDS_MAX = 3072;         // ... filled to 3/4 at most
constexpr int LV_DIRECT_MAX = LV_LDS_SLOTS;
constexpr int LV_POOL_THREADS = 512;     // bin 2
constexpr int LV_POOL_MAX = 1024;
constexpr size_t LV_POOL_BYTES = (size_t)256 << 20;
constexpr int LV_TRY_PROBES = 64;
constexpr int LV_EMPTY = -1;
constexpr int LV_NONE = INT_MAX;
constexpr int64_t LV_MAX_NNZ = 0x7fffff00LL;   // hipcub counts items in int
constexpr int64_t LV_MAX_N = 0x7ffffff0LL;
constexpr unsigned LV_ERR_TABLE_FULL = 1u;

struct LvGraph {
  const long long *ptr;
  const int32_t *adj;
  const uint16_t *codes;      // level 0: weight of entry e = wq[codes[e]]
  const long long *wq;
  const long long *w;         // coarse levels
};
template <bool L0> __device__ __forceinline__ long long lv_weight(const LvGraph &g, long long e) { return L0 ? g.wq[g.codes[e]] : g.w[e]; }

struct LvState {
  const int32_t *comm;
  const long long *tot;
  const int32_t *size;
  const long long *k;
  int32_t *next;
  double res, m2;
  unsigned *err;
};

// what the host reads back: the first 32 bytes once per iteration
struct LvRecord {
  unsigned long long moved;
  long long in;
  unsigned long long s_lo, s_hi;
  unsigned err, bad;
  unsigned long long m2;
  long long maxdeg;
  unsigned count[LV_BUCKETS], cursor[LV_BUCKETS];
  unsigned over;              // bin 2: rows of the current sub-round whose communities did not fit the LDS table
};
struct LvOffsets { int at[LV_BUCKETS + 1]; };

__device__ __forceinline__ long long lv_shfl64(long long v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)((unsigned long long)v >> 32), src);
  return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ long long lv_wave_sum(long long v) {
  for (int o = 32; o > 0; o >>= 1) v += lv_shfl64(v, (int)((threadIdx.x & 63) ^ o));
  return v;
}
__device__ __forceinline__ uint32_t lv_class(int64_t v, uint32_t seed, int level) {
  return (uint32_t)((((uint64_t)v * 2654435761ull + (uint64_t)seed * 40503ull + (uint64_t)level) >> 7) & 7);
}

// ---- the decision ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double lv_gain(long long w, long long t, double kv, const LvState &s) {
  const double a = s.res * (double)t;
  const double b = a * kv;
  const double c = b / s.m2;
  return (double)w - c;
}
struct LvBest { double g; int c; };
__device__ __forceinline__ bool lv_better(const LvBest &a, const LvBest &b) {      // a before b in (gain descending, id ascending)
  return a.c != LV_NONE && (b.c == LV_NONE || a.g > b.g || (a.g == b.g && a.c < b.c));
}
__device__ __forceinline__ void lv_consider(LvBest &best, int c, long long w, int C, int size_c, double stay, double kv, const LvState &s) {
  LvBest cand;
  cand.g = lv_gain(w, s.tot[c], kv, s);
  cand.c = c;
  if (!(cand.g > stay)) return;
  if (size_c == 1 && c > C && s.size[c] == 1) return;                               // two lone vertices must not swap for ever
  if (lv_better(cand, best)) best = cand;
}
__device__ __forceinline__ LvBest lv_wave_best(LvBest b) {
  for (int o = 32; o > 0; o >>= 1) {
    LvBest other;
    other.g = __shfl_xor(b.g, o);
    other.c = __shfl_xor(b.c, o);
    if (lv_better(other, b)) b = other;
  }
  return b;
}

// ---- k_lv_validate: before anything indexes by a neighbour id or a code ----------------------------------------------------------------
// ptr[0] = 0 and ptr[n] = nnz were read by the host.  One wave per row: row pointers do not decrease and stay inside [0, nnz]; neighbours
// are in range, ascending, distinct and not the row itself; codes are below n_values.  Symmetry is NOT checked.
__global__ __launch_bounds__(LV_THREADS) void k_lv_validate(const long long *__restrict__ ptr, const int32_t *__restrict__ adj,
                                                            const uint16_t *__restrict__ codes, const uint16_t *__restrict__ loops, int64_t n,
                                                            long long nnz, int n_values, unsigned *__restrict__ bad) {
  const int lane = threadIdx.x & 63;
  const int64_t v = (int64_t)blockIdx.x * LV_WAVES + (threadIdx.x >> 6);
  if (v >= n) return;
  const long long p0 = ptr[v], p1 = ptr[v + 1];
  bool wrong = p0 < 0 || p1 < p0 || p1 > nnz;
  if (!wrong) {
    for (long long e = p0 + lane; e < p1; e += 64) {
      const int32_t a = adj[e];
      if (a < 0 || a >= n || a == v || (int)codes[e] >= n_values) wrong = true;
      if (e > p0 && adj[e - 1] >= a) wrong = true;
    }
  }
  if (lane == 0 && loops && loops[v] != 0xFFFF && (int)loops[v] >= n_values) wrong = true;
  if (wrong) atomicOr(bad, 1u);
}

// ---- setup of a level: strengths, singletons, class and degree bin ---------------------------------------------------------------------
template <bool L0>
__global__ __launch_bounds__(LV_THREADS) void k_lv_setup(LvGraph g, const uint16_t *__restrict__ loop_codes, long long *__restrict__ loop, int64_t n,
                                                         uint32_t seed, int level, int direct, long long *__restrict__ k, long long *__restrict__ tot,
                                                         int32_t *__restrict__ comm, int32_t *__restrict__ size, uint8_t *__restrict__ bucket,
                                                         LvRecord *__restrict__ rec) {
  const int lane = threadIdx.x & 63;
  const int64_t v = (int64_t)blockIdx.x * LV_WAVES + (threadIdx.x >> 6);
  if (v >= n) return;
  const long long p0 = g.ptr[v], deg = g.ptr[v + 1] - p0;
  long long sum = 0;
  for (long long e = lane; e < deg; e += 64) sum += lv_weight<L0>(g, p0 + e);
  sum = lv_wave_sum(sum);
  if (lane != 0) return;
  long long lp;
  if (L0) {
    lp = (loop_codes && loop_codes[v] != 0xFFFF) ? g.wq[loop_codes[v]] : 0;
    loop[v] = lp;
  } else {
    lp = loop[v];
  }
  const long long kv = 2 * lp + sum;
  k[v] = kv;
  tot[v] = kv;
  comm[v] = (int32_t)v;
  size[v] = 1;
  const int bin = deg <= LV_WAVE_MAX ? 0 : (direct || deg <= LV_LDS_MAX) ? 1 : 2;
  const int b = (int)lv_class(v, seed, level) * LV_BINS + bin;
  bucket[v] = (uint8_t)b;
  atomicAdd(&rec->count[b], 1u);
  atomicAdd(&rec->m2, (unsigned long long)kv);
  atomicMax(&rec->maxdeg, deg);
}
__global__ __launch_bounds__(LV_THREADS) void k_lv_scatter(const uint8_t *__restrict__ bucket, int64_t n, LvOffsets off, LvRecord *__restrict__ rec,
                                                           int32_t *__restrict__ list) {
  const int64_t v = (int64_t)blockIdx.x * LV_THREADS + threadIdx.x;
  if (v >= n) return;
  const int b = bucket[v];
  list[off.at[b] + (int)atomicAdd(&rec->cursor[b], 1u)] = (int32_t)v;
}
__global__ __launch_bounds__(LV_THREADS) void k_lv_iota(int32_t *__restrict__ out, int64_t n) {
  const int64_t v = (int64_t)blockIdx.x * LV_THREADS + threadIdx.x;
  if (v < n) out[v] = (int32_t)v;
}

// ---- k_lv_decide, bin 0: a wave per row, a lane per entry --------------------------------------------------------------------------------
template <bool L0>
__global__ __launch_bounds__(LV_THREADS) void k_lv_decide_wave(LvGraph g, LvState s, const int32_t *__restrict__ list, int count) {
  const int lane = threadIdx.x & 63;
  const int r = (int)blockIdx.x * LV_WAVES + (int)(threadIdx.x >> 6);
  if (r >= count) return;
  const int32_t v = list[r];
  const long long p0 = g.ptr[v];
  const int deg = (int)(g.ptr[v + 1] - p0);                      // <= 64
  const int C = s.comm[v];
  const long long kv_i = s.k[v];
  const double kv = (double)kv_i;
  int c = LV_EMPTY;
  long long w = 0;
  if (lane < deg) {
    c = s.comm[g.adj[p0 + lane]];
    w = lv_weight<L0>(g, p0 + lane);
  }
  long long sum = 0;
  bool head = lane < deg;
  for (int j = 0; j < deg; ++j) {                                // wave-uniform bound
    const int cj = __shfl(c, j);
    const long long wj = lv_shfl64(w, j);
    if (cj == c) {
      sum += wj;
      if (j < lane) head = false;
    }
  }
  const unsigned long long own = __ballot(lane < deg && c == C);
  const long long w_own_any = lv_shfl64(sum, own ? __ffsll((long long)own) - 1 : 0);
  const long long w_own = own ? w_own_any : 0;
  const double stay = lv_gain(w_own, s.tot[C] - kv_i, kv, s);
  const int size_c = s.size[C];
  LvBest best;
  best.g = 0.0;
  best.c = LV_NONE;
  if (head && c != C) lv_consider(best, c, sum, C, size_c, stay, kv, s);
  best = lv_wave_best(best);
  if (lane == 0) s.next[v] = best.c == LV_NONE ? C : best.c;
}

// ---- k_lv_decide, bins 1 and 2: a workgroup per row and a table -----------------------------------------------------------------------------
// MODE 0: open addressing in LDS; MODE 1: LDS indexed by the community id (levels of <= LV_DIRECT_MAX vertices); MODE 2: open addressing in the
// workspace, one table of `stride` slots per workgroup.  In MODE 2 the table is read and written with agent-scope accesses only and the
// phases are separated by an agent fence, so no lane reads a stale L1 line of a slot another wave's atomic has changed.
// MODE 3 is how a bin-2 row is tried first: the LDS table whatever the row's length, because after the first sub-rounds a long row has
// far fewer neighbouring communities than entries.  A probe sequence is cut at LV_TRY_PROBES; a row that meets the cut decides nothing and
// is appended to over_list, which a MODE 2 launch then takes (its row count read from *count_ptr).  Sums are integers, so which table a
// row used does not show in the result.
template <int MODE> __device__ __forceinline__ int lv_ld(const int *p) {
  return MODE == 2 ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *p;
}
template <int MODE> __device__ __forceinline__ unsigned long long lv_ld(const unsigned long long *p) {
  return MODE == 2 ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *p;
}
template <int MODE> __device__ __forceinline__ void lv_phase() {
  if (MODE == 2) __threadfence();
  __syncthreads();
}
__device__ __forceinline__ unsigned lv_hash(int c, int mask) { return (unsigned)(((uint64_t)(uint32_t)c * 0x9E3779B97F4A7C15ull) >> 32) & (unsigned)mask; }

template <bool L0, int MODE>
__global__ __launch_bounds__(MODE == 2 ? LV_POOL_THREADS : LV_THREADS) void k_lv_decide_table(LvGraph g, LvState s, const int32_t *__restrict__ list,
                                                                                              int count, int n, int *gkeys, unsigned long long *gvals,
                                                                                              long long stride, const unsigned *count_ptr,
                                                                                              int32_t *over_list, unsigned *over_count) {
  constexpr int SLOTS = MODE == 2 ? 1 : LV_LDS_SLOTS;
  constexpr bool TRY = MODE == 3;
  __shared__ int s_over;
  if (MODE == 2 && count_ptr) count = min(count, (int)*count_ptr);
  __shared__ int skeys[SLOTS];
  __shared__ unsigned long long svals[SLOTS];
  __shared__ double red_g[LV_POOL_THREADS / 64];
  __shared__ int red_c[LV_POOL_THREADS / 64];
  int *keys = MODE == 2 ? gkeys + (long long)blockIdx.x * stride : skeys;
  unsigned long long *vals = MODE == 2 ? gvals + (long long)blockIdx.x * stride : svals;
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6;
  const long long cap = MODE == 2 ? stride : LV_LDS_SLOTS;
  for (int r = blockIdx.x; r < count; r += gridDim.x) {
    const int32_t v = list[r];
    const long long p0 = g.ptr[v], deg = g.ptr[v + 1] - p0;
    const int C = s.comm[v];
    const long long kv_i = s.k[v];
    const double kv = (double)kv_i;
    long long T = n;
    if (MODE != 1) {
      T = 64;
      while (T < 2 * deg && T < cap) T <<= 1;
    }
    const int mask = (int)(T - 1);
    const long long probes = TRY ? (long long)LV_TRY_PROBES : T;
    if (TRY && tid == 0) s_over = 0;
    for (long long i = tid; i < T; i += nt) {
      if (MODE == 2) {
        __hip_atomic_store(&keys[i], LV_EMPTY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&vals[i], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        keys[i] = LV_EMPTY;
        vals[i] = 0ull;
      }
    }
    lv_phase<MODE>();
    for (long long e = tid; e < deg; e += nt) {
      if (TRY && *(volatile int *)&s_over) break;                // the row goes to the workspace table: nothing more to add here
      const int c = s.comm[g.adj[p0 + e]];
      const long long w = lv_weight<L0>(g, p0 + e);
      long long slot = -1;
      if (MODE == 1) {
        slot = c;
        keys[c] = c;
      } else {
        unsigned h = lv_hash(c, mask);
        for (long long t = 0; t < probes; ++t) {                 // bounded by the table size (MODE 3: by LV_TRY_PROBES)
          const int old = atomicCAS(&keys[h], LV_EMPTY, c);
          if (old == LV_EMPTY || old == c) { slot = h; break; }
          h = (h + 1) & (unsigned)mask;
        }
      }
      if (slot >= 0) atomicAdd(&vals[slot], (unsigned long long)w);
      else if (TRY) s_over = 1;
      else atomicOr(s.err, LV_ERR_TABLE_FULL);
    }
    lv_phase<MODE>();
    if (TRY && s_over) {                                         // block-uniform: read behind the barrier
      if (tid == 0) over_list[atomicAdd(over_count, 1u)] = v;
      __syncthreads();                                           // s_over is cleared for the next row only after everyone has read it
      continue;
    }
    long long w_own = 0;
    if (MODE == 1) {
      if (keys[C] == C) w_own = (long long)vals[C];
    } else {
      unsigned h = lv_hash(C, mask);
      for (long long t = 0; t < T; ++t) {
        const int kk = lv_ld<MODE>(&keys[h]);
        if (kk == C) { w_own = (long long)lv_ld<MODE>(&vals[h]); break; }
        if (kk == LV_EMPTY) break;
        h = (h + 1) & (unsigned)mask;
      }
    }
    const double stay = lv_gain(w_own, s.tot[C] - kv_i, kv, s);
    const int size_c = s.size[C];
    LvBest best;
    best.g = 0.0;
    best.c = LV_NONE;
    for (long long i = tid; i < T; i += nt) {
      const int c = lv_ld<MODE>(&keys[i]);
      if (c != LV_EMPTY && c != C) lv_consider(best, c, (long long)lv_ld<MODE>(&vals[i]), C, size_c, stay, kv, s);
    }
    best = lv_wave_best(best);
    if (lane == 0) { red_g[wave] = best.g; red_c[wave] = best.c; }
    __syncthreads();
    if (tid == 0) {
      for (int q = 1; q < nt / 64; ++q) {
        LvBest other;
        other.g = red_g[q];
        other.c = red_c[q];
        if (lv_better(other, best)) best = other;
      }
      s.next[v] = best.c == LV_NONE ? C : best.c;
    }
    lv_phase<MODE>();                                            // the table and red_* are reused by the next row
  }
}

// ---- k_lv_apply: the moves of one class (a second launch: a fused kernel would read comm while it changes) -------------------------------
__global__ __launch_bounds__(LV_THREADS) void k_lv_apply(const int32_t *__restrict__ list, int count, const int32_t *__restrict__ next,
                                                         const long long *__restrict__ k, int32_t *__restrict__ comm, long long *__restrict__ tot,
                                                         int32_t *__restrict__ size, LvRecord *__restrict__ rec) {
  const int i = (int)blockIdx.x * LV_THREADS + (int)threadIdx.x;
  bool moved = false;
  if (i < count) {
    const int32_t v = list[i];
    const int32_t to = next[v], from = comm[v];
    if (to != from) {
      moved = true;
      const unsigned long long kv = (unsigned long long)k[v];
      atomicAdd(reinterpret_cast<unsigned long long *>(&tot[from]), 0ull - kv);
      atomicAdd(reinterpret_cast<unsigned long long *>(&tot[to]), kv);
      atomicSub(&size[from], 1);
      atomicAdd(&size[to], 1);
      comm[v] = to;
    }
  }
  const unsigned long long m = __ballot(moved);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&rec->moved, (unsigned long long)__popcll(m));
}

// ---- k_lv_internal: IN (exact int64) and S = sum tot^2 (exact, two 64-bit limbs), one set of atomics per workgroup -----------------------
template <bool L0>
__global__ __launch_bounds__(LV_THREADS) void k_lv_internal(LvGraph g, const long long *__restrict__ loop, const int32_t *__restrict__ comm,
                                                            const long long *__restrict__ tot, int64_t n, LvRecord *__restrict__ rec) {
  __shared__ long long s_in[LV_WAVES];
  __shared__ unsigned long long s_lo[LV_WAVES], s_hi[LV_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long in = 0;
  unsigned long long lo = 0, hi = 0;
  for (int64_t v = (int64_t)blockIdx.x * LV_WAVES + wave; v < n; v += (int64_t)gridDim.x * LV_WAVES) {
    const long long p0 = g.ptr[v], deg = g.ptr[v + 1] - p0;
    const int C = comm[v];
    for (long long e = lane; e < deg; e += 64)
      if (comm[g.adj[p0 + e]] == C) in += lv_weight<L0>(g, p0 + e);
    if (lane == 0) {
      in += 2 * loop[v];
      const unsigned long long t = (unsigned long long)tot[v];
      const unsigned long long q = t * t;
      lo += q;
      hi += __umul64hi(t, t) + (lo < q ? 1ull : 0ull);
    }
  }
  in = lv_wave_sum(in);
  if (lane == 0) { s_in[wave] = in; s_lo[wave] = lo; s_hi[wave] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < LV_WAVES; ++q) {
      in += s_in[q];
      lo += s_lo[q];
      hi += s_hi[q] + (lo < s_lo[q] ? 1ull : 0ull);
    }
    if (in) atomicAdd(reinterpret_cast<unsigned long long *>(&rec->in), (unsigned long long)in);
    if (lo) {
      const unsigned long long old = atomicAdd(&rec->s_lo, lo);
      if (old + lo < old) ++hi;                                  // this add wrapped the low limb
    }
    if (hi) atomicAdd(&rec->s_hi, hi);
  }
}

// ---- aggregation -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LV_THREADS) void k_lv_flags(const int32_t *__restrict__ size, int64_t n, long long *__restrict__ flag) {
  const int64_t c = (int64_t)blockIdx.x * LV_THREADS + threadIdx.x;
  if (c <= n) flag[c] = (c < n && size[c] > 0) ? 1 : 0;
}
__global__ __launch_bounds__(LV_THREADS) void k_lv_member(int32_t *__restrict__ member, int64_t n0, const int32_t *__restrict__ comm,
                                                          const long long *__restrict__ newid) {
  const int64_t i = (int64_t)blockIdx.x * LV_THREADS + threadIdx.x;
  if (i < n0) member[i] = (int32_t)newid[comm[member[i]]];
}
// per row: the number of entries that leave the row's community, and 2 loop + internal weight into the community's accumulator
template <bool L0>
__global__ __launch_bounds__(LV_THREADS) void k_lv_cross_count(LvGraph g, const long long *__restrict__ loop, const int32_t *__restrict__ comm,
                                                               const long long *__restrict__ newid, int64_t n, long long *__restrict__ cnt,
                                                               long long *__restrict__ acc) {
  const int lane = threadIdx.x & 63;
  const int64_t v = (int64_t)blockIdx.x * LV_WAVES + (threadIdx.x >> 6);
  if (v >= n) return;
  const long long p0 = g.ptr[v], deg = g.ptr[v + 1] - p0;
  const int C = comm[v];
  long long cross = 0, inner = 0;
  for (long long e = lane; e < deg; e += 64) {
    if (comm[g.adj[p0 + e]] == C) inner += lv_weight<L0>(g, p0 + e);
    else ++cross;
  }
  cross = lv_wave_sum(cross);
  inner = lv_wave_sum(inner);
  if (lane == 0) {
    cnt[v] = cross;
    atomicAdd(reinterpret_cast<unsigned long long *>(&acc[newid[C]]), (unsigned long long)(2 * loop[v] + inner));
  }
}
template <bool L0>
__global__ __launch_bounds__(LV_THREADS) void k_lv_emit(LvGraph g, const int32_t *__restrict__ comm, const long long *__restrict__ newid, int64_t n,
                                                        const long long *__restrict__ off, long long capacity, unsigned long long *__restrict__ keys,
                                                        long long *__restrict__ vals) {
  const int lane = threadIdx.x & 63;
  const int64_t v = (int64_t)blockIdx.x * LV_WAVES + (threadIdx.x >> 6);
  if (v >= n) return;
  const long long p0 = g.ptr[v], deg = g.ptr[v + 1] - p0;
  const int C = comm[v];
  const unsigned long long a = (unsigned long long)newid[C] << 32;
  long long at = off[v];
  for (long long e0 = 0; e0 < deg; e0 += 64) {                   // wave-uniform bound
    const long long e = e0 + lane;
    int c = C;
    if (e < deg) c = comm[g.adj[p0 + e]];
    const unsigned long long m = __ballot(c != C);
    if (c != C) {
      const long long slot = at + __popcll(m & ((1ull << lane) - 1));
      if (slot < capacity) {
        keys[slot] = a | (unsigned long long)newid[c];
        vals[slot] = lv_weight<L0>(g, p0 + e);
      }
    }
    at += __popcll(m);
  }
}
__global__ __launch_bounds__(LV_THREADS) void k_lv_coarse_entries(const unsigned long long *__restrict__ keys, const long long *__restrict__ sums,
                                                                  long long runs, int32_t *__restrict__ adj, long long *__restrict__ w) {
  const long long i = (long long)blockIdx.x * LV_THREADS + threadIdx.x;
  if (i < runs) {
    adj[i] = (int32_t)(uint32_t)keys[i];
    w[i] = sums[i];
  }
}
__global__ __launch_bounds__(LV_THREADS) void k_lv_coarse_rows(const unsigned long long *__restrict__ keys, long long runs, int64_t nc,
                                                               long long *__restrict__ ptr, const long long *__restrict__ acc, long long *__restrict__ loop) {
  const int64_t v = (int64_t)blockIdx.x * LV_THREADS + threadIdx.x;
  if (v > nc) return;
  const unsigned long long want = (unsigned long long)v << 32;
  long long lo = 0, hi = runs;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (keys[mid] < want) lo = mid + 1; else hi = mid;
  }
  ptr[v] = lo;
  if (v < nc) loop[v] = acc[v] / 2;                              // every internal entry was counted from both ends
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
inline size_t lv_temp_bytes(int64_t n, int64_t nnz) {
  size_t a = 0, b = 0, c = 0;
  const int items = (int)std::max<int64_t>(nnz, 1);
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, (const long long *)nullptr,
                                           (long long *)nullptr, items, 0, 64, nullptr);
  (void)hipcub::DeviceReduce::ReduceByKey(nullptr, b, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, (const long long *)nullptr,
                                          (long long *)nullptr, (long long *)nullptr, hipcub::Sum(), items, nullptr);
  c = scan_i64_bytes(n + 1);
  return std::max(a, std::max(b, c));
}
inline long long lv_pow2_at_least(long long x) {
  long long t = 64;
  while (t < x) t <<= 1;
  return t;
}

struct LvLayout {
  size_t rec, wq, k, tot, loop0, loop_a, loop_b, acc, cnt, off, newid, ptr_a, ptr_b, comm, next, size, list, over, member, bucket;
  size_t adj_a, adj_b, w_a, w_b, keys_a, keys_b, vals_a, vals_b, temp, temp_bytes, pool, pool_bytes, total;
};
LvLayout lv_layout(int64_t n, int64_t nnz) {
  LvLayout L;
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t o = at; at += up256(bytes); return o; };
  const size_t nv = (size_t)n, ne = (size_t)nnz;
  L.rec = take(sizeof(LvRecord));
  L.wq = take(65536 * 8);
  L.k = take(nv * 8); L.tot = take(nv * 8); L.loop0 = take(nv * 8); L.loop_a = take(nv * 8); L.loop_b = take(nv * 8); L.acc = take(nv * 8);
  L.cnt = take((nv + 1) * 8); L.off = take((nv + 1) * 8); L.newid = take((nv + 1) * 8); L.ptr_a = take((nv + 1) * 8); L.ptr_b = take((nv + 1) * 8);
  L.comm = take(nv * 4); L.next = take(nv * 4); L.size = take(nv * 4); L.list = take(nv * 4); L.over = take(nv * 4); L.member = take(nv * 4); L.bucket = take(nv);
  L.adj_a = take(ne * 4); L.adj_b = take(ne * 4); L.w_a = take(ne * 8); L.w_b = take(ne * 8);
  L.keys_a = take(ne * 8); L.keys_b = take(ne * 8); L.vals_a = take(ne * 8); L.vals_b = take(ne * 8);
  L.temp_bytes = lv_temp_bytes(n, nnz);
  L.temp = take(L.temp_bytes);
  const int64_t deg_bound = std::min<int64_t>(n > 0 ? n - 1 : 0, nnz);
  L.pool_bytes = 0;
  if (deg_bound > LV_LDS_MAX && n > LV_DIRECT_MAX) {
    const size_t one = (size_t)lv_pow2_at_least(2 * deg_bound) * 12 + 256;
    L.pool_bytes = std::max(one, std::min(one * LV_POOL_MAX, LV_POOL_BYTES));
  }
  L.pool = take(L.pool_bytes);
  L.total = at + 256;
  return L;
}

double lv_quality(long long in, unsigned long long s_lo, unsigned long long s_hi, unsigned long long m2, double res) {
  const unsigned __int128 s = ((unsigned __int128)s_hi << 64) | s_lo;
  const double m2d = (double)m2;
  const double a = (double)in / m2d;
  const double b = (double)s / (m2d * m2d);
  return a - res * b;
}

inline unsigned lv_blocks(int64_t items, int per_block) { return (unsigned)std::max<int64_t>(ceil_div(items, per_block), 1); }

template <bool L0>
int lv_level(const LvGraph &g, const uint16_t *d_loop_codes, long long *d_loop, int64_t n, int level, uint32_t seed, double res, char *work,
             const LvLayout &L, unsigned long long m2_expected, bool *moved_any, int *iterations, double *q_out, unsigned long long *m2_out,
             hipStream_t stream) {
  LvRecord *d_rec = at_bytes<LvRecord>(work, L.rec);
  long long *d_k = at_bytes<long long>(work, L.k), *d_tot = at_bytes<long long>(work, L.tot);
  int32_t *d_comm = at_bytes<int32_t>(work, L.comm), *d_next = at_bytes<int32_t>(work, L.next), *d_size = at_bytes<int32_t>(work, L.size);
  int32_t *d_list = at_bytes<int32_t>(work, L.list), *d_over = at_bytes<int32_t>(work, L.over);
  uint8_t *d_bucket = at_bytes<uint8_t>(work, L.bucket);
  const int direct = n <= LV_DIRECT_MAX ? 1 : 0;
  LvRecord rec;
  DA_HIP_TRY(hipMemsetAsync(d_rec, 0, sizeof(LvRecord), stream));
  hipLaunchKernelGGL(k_lv_setup<L0>, dim3(lv_blocks(n, LV_WAVES)), dim3(LV_THREADS), 0, stream, g, d_loop_codes, d_loop, n, seed, level, direct, d_k, d_tot,
                     d_comm, d_size, d_bucket, d_rec);
  DA_HIP_TRY(hipGetLastError());
  DA_HIP_TRY(hipMemcpyAsync(&rec, d_rec, sizeof(LvRecord), hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipStreamSynchronize(stream));
  *m2_out = rec.m2;
  *moved_any = false;
  *iterations = 0;
  if (rec.m2 == 0) return DA_OK;                                  // level 0 without any weight: the caller returns singletons
  if (level > 0 && rec.m2 != m2_expected) return fail(DA_ERR_HIP, "device Louvain: the total weight changed under aggregation (internal error)");
  if (rec.m2 >= (1ull << 62)) return fail(DA_ERR_UNSUPPORTED, "device Louvain: total weight too large for exact 64-bit sums");
  LvOffsets off;
  off.at[0] = 0;
  for (int b = 0; b < LV_BUCKETS; ++b) off.at[b + 1] = off.at[b] + (int)rec.count[b];
  if (off.at[LV_BUCKETS] != n) return fail(DA_ERR_HIP, "device Louvain: class lists do not cover the level (internal error)");
  hipLaunchKernelGGL(k_lv_scatter, dim3(lv_blocks(n, LV_THREADS)), dim3(LV_THREADS), 0, stream, d_bucket, n, off, d_rec, d_list);
  DA_HIP_TRY(hipGetLastError());
  // bin 2: one table per pool workgroup, sized from this level's largest degree
  long long stride = 0;
  int pool = 0;
  int *d_pool_keys = nullptr;
  unsigned long long *d_pool_vals = nullptr;
  int any_pool = 0;
  for (int c = 0; c < LV_CLASSES; ++c) any_pool = std::max(any_pool, (int)rec.count[c * LV_BINS + 2]);
  if (any_pool) {
    stride = lv_pow2_at_least(2 * rec.maxdeg);
    const size_t one = (size_t)stride * 12 + 256;
    if (L.pool_bytes < one) return fail(DA_ERR_HIP, "device Louvain: the table pool is smaller than one table (internal error)");
    pool = (int)std::min<size_t>(std::min<size_t>((L.pool_bytes - 256) / ((size_t)stride * 12), LV_POOL_MAX), (size_t)any_pool);
    if (pool < 1) pool = 1;
    d_pool_keys = at_bytes<int>(work, L.pool);
    d_pool_vals = at_bytes<unsigned long long>(work, L.pool + up256((size_t)pool * (size_t)stride * 4));
  }
  LvState s;
  s.comm = d_comm; s.tot = d_tot; s.size = d_size; s.k = d_k; s.next = d_next; s.res = res; s.m2 = (double)rec.m2; s.err = &d_rec->err;
  const unsigned sweep_blocks = (unsigned)std::min<int64_t>(lv_blocks(n, LV_WAVES), 4096);
  auto quality = [&](double *q, unsigned long long *moved) -> int {
    hipLaunchKernelGGL(k_lv_internal<L0>, dim3(sweep_blocks), dim3(LV_THREADS), 0, stream, g, d_loop, d_comm, d_tot, n, d_rec);
    DA_HIP_TRY(hipGetLastError());
    DA_HIP_TRY(hipMemcpyAsync(&rec, d_rec, 40, hipMemcpyDeviceToHost, stream));        // moved, IN, S, err
    DA_HIP_TRY(hipStreamSynchronize(stream));
    if (rec.err) return fail(DA_ERR_HIP, "device Louvain: a neighbour-community table overflowed (internal error)");
    *q = lv_quality(rec.in, rec.s_lo, rec.s_hi, rec.m2, res);
    *moved = rec.moved;
    return DA_OK;
  };
  int rc;
  double q_prev = 0.0, q = 0.0;
  unsigned long long moved = 0;
  const unsigned long long m2 = rec.m2;
  rec.m2 = m2;
  if ((rc = quality(&q_prev, &moved)) != DA_OK) return rc;
  q = q_prev;
  for (int it = 0; it < LV_MAX_ITERATIONS; ++it) {
    DA_HIP_TRY(hipMemsetAsync(d_rec, 0, 32, stream));
    for (int c = 0; c < LV_CLASSES; ++c) {
      const int *at = off.at + c * LV_BINS;
      const int n0 = at[1] - at[0], n1 = at[2] - at[1], n2 = at[3] - at[2];
      if (n0 + n1 + n2 == 0) continue;
      if (n0)
        hipLaunchKernelGGL(k_lv_decide_wave<L0>, dim3(lv_blocks(n0, LV_WAVES)), dim3(LV_THREADS), 0, stream, g, s, d_list + at[0], n0);
      if (n1) {
        const unsigned blocks = (unsigned)std::min(n1, 8192);
        if (direct)
          hipLaunchKernelGGL((k_lv_decide_table<L0, 1>), dim3(blocks), dim3(LV_THREADS), 0, stream, g, s, d_list + at[1], n1, (int)n, (int *)nullptr,
                             (unsigned long long *)nullptr, 0LL, (const unsigned *)nullptr, (int32_t *)nullptr, (unsigned *)nullptr);
        else
          hipLaunchKernelGGL((k_lv_decide_table<L0, 0>), dim3(blocks), dim3(LV_THREADS), 0, stream, g, s, d_list + at[1], n1, (int)n, (int *)nullptr,
                             (unsigned long long *)nullptr, 0LL, (const unsigned *)nullptr, (int32_t *)nullptr, (unsigned *)nullptr);
      }
      if (n2) {                                                  // the LDS table first; the rows it cannot hold go to the workspace tables
        DA_HIP_TRY(hipMemsetAsync(&d_rec->over, 0, 4, stream));
        hipLaunchKernelGGL((k_lv_decide_table<L0, 3>), dim3((unsigned)std::min(n2, 8192)), dim3(LV_THREADS), 0, stream, g, s, d_list + at[2], n2, (int)n,
                           (int *)nullptr, (unsigned long long *)nullptr, 0LL, (const unsigned *)nullptr, d_over, &d_rec->over);
        hipLaunchKernelGGL((k_lv_decide_table<L0, 2>), dim3((unsigned)std::min(n2, pool)), dim3(LV_POOL_THREADS), 0, stream, g, s, d_over, n2, (int)n,
                           d_pool_keys, d_pool_vals, stride, (const unsigned *)&d_rec->over, (int32_t *)nullptr, (unsigned *)nullptr);
      }
      hipLaunchKernelGGL(k_lv_apply, dim3(lv_blocks(n0 + n1 + n2, LV_THREADS)), dim3(LV_THREADS), 0, stream, d_list + at[0], n0 + n1 + n2, d_next, d_k,
                         d_comm, d_tot, d_size, d_rec);
    }
    DA_HIP_TRY(hipGetLastError());
    rec.m2 = m2;
    if ((rc = quality(&q, &moved)) != DA_OK) return rc;
    ++*iterations;
    if (moved == 0) break;
    *moved_any = true;
    if (!(q > q_prev)) break;                                     // the moves are kept
    q_prev = q;
  }
  *q_out = q;
  return DA_OK;
}

// communities -> the next level's graph in (d_ptr, d_adj, d_w, d_loop); returns its vertex and entry counts
template <bool L0>
int lv_aggregate(const LvGraph &g, const long long *d_loop, int64_t n, int64_t n0, int64_t nnz_cap, char *work, const LvLayout &L, long long *d_ptr,
                 int32_t *d_adj, long long *d_w, long long *d_loop_out, int64_t *nc_out, int64_t *nnz_out, hipStream_t stream) {
  int32_t *d_comm = at_bytes<int32_t>(work, L.comm), *d_size = at_bytes<int32_t>(work, L.size), *d_member = at_bytes<int32_t>(work, L.member);
  long long *d_cnt = at_bytes<long long>(work, L.cnt), *d_off = at_bytes<long long>(work, L.off), *d_newid = at_bytes<long long>(work, L.newid);
  long long *d_acc = at_bytes<long long>(work, L.acc);
  unsigned long long *keys_a = at_bytes<unsigned long long>(work, L.keys_a), *keys_b = at_bytes<unsigned long long>(work, L.keys_b);
  long long *vals_a = at_bytes<long long>(work, L.vals_a), *vals_b = at_bytes<long long>(work, L.vals_b);
  void *temp = work + L.temp;
  size_t tb = L.temp_bytes;
  hipLaunchKernelGGL(k_lv_flags, dim3(lv_blocks(n + 1, LV_THREADS)), dim3(LV_THREADS), 0, stream, d_size, n, d_cnt);
  DA_HIP_TRY(hipGetLastError());
  DA_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(temp, tb, d_cnt, d_newid, (int)(n + 1), stream));
  long long nc = 0, cross = 0, runs = 0;
  DA_HIP_TRY(hipMemcpyAsync(&nc, d_newid + n, 8, hipMemcpyDeviceToHost, stream));
  hipLaunchKernelGGL(k_lv_member, dim3(lv_blocks(n0, LV_THREADS)), dim3(LV_THREADS), 0, stream, d_member, n0, d_comm, d_newid);
  DA_HIP_TRY(hipMemsetAsync(d_acc, 0, (size_t)n * 8, stream));
  DA_HIP_TRY(hipMemsetAsync(d_cnt + n, 0, 8, stream));
  hipLaunchKernelGGL(k_lv_cross_count<L0>, dim3(lv_blocks(n, LV_WAVES)), dim3(LV_THREADS), 0, stream, g, d_loop, d_comm, d_newid, n, d_cnt, d_acc);
  DA_HIP_TRY(hipGetLastError());
  tb = L.temp_bytes;
  DA_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(temp, tb, d_cnt, d_off, (int)(n + 1), stream));
  DA_HIP_TRY(hipMemcpyAsync(&cross, d_off + n, 8, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipStreamSynchronize(stream));
  if (nc < 1 || nc > n || cross < 0 || cross > nnz_cap) return fail(DA_ERR_HIP, "device Louvain: aggregation counts out of range (internal error)");
  if (cross > 0) {
    hipLaunchKernelGGL(k_lv_emit<L0>, dim3(lv_blocks(n, LV_WAVES)), dim3(LV_THREADS), 0, stream, g, d_comm, d_newid, n, d_off, cross, keys_a, vals_a);
    DA_HIP_TRY(hipGetLastError());
    tb = L.temp_bytes;
    DA_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(temp, tb, keys_a, keys_b, vals_a, vals_b, (int)cross, 0, 32 + bits_for(nc), stream));
    tb = L.temp_bytes;
    DA_HIP_TRY(hipcub::DeviceReduce::ReduceByKey(temp, tb, keys_b, keys_a, vals_b, vals_a, d_cnt, hipcub::Sum(), (int)cross, stream));
    DA_HIP_TRY(hipMemcpyAsync(&runs, d_cnt, 8, hipMemcpyDeviceToHost, stream));
    DA_HIP_TRY(hipStreamSynchronize(stream));
    if (runs < 0 || runs > cross) return fail(DA_ERR_HIP, "device Louvain: coarse edge count out of range (internal error)");
    hipLaunchKernelGGL(k_lv_coarse_entries, dim3(lv_blocks(runs, LV_THREADS)), dim3(LV_THREADS), 0, stream, keys_a, vals_a, runs, d_adj, d_w);
  }
  hipLaunchKernelGGL(k_lv_coarse_rows, dim3(lv_blocks(nc + 1, LV_THREADS)), dim3(LV_THREADS), 0, stream, keys_a, runs, (int64_t)nc, d_ptr, d_acc, d_loop_out);
  DA_HIP_TRY(hipGetLastError());
  *nc_out = nc;
  *nnz_out = runs;
  return DA_OK;
}

}  // namespace

// sizes are asked for before anything is validated: arguments outside what the call accepts are clamped to its limits (the call refuses them),
// so the int item counts of the hipcub size queries below never wrap
size_t louvain_device_workspace_bytes(int64_t n, int64_t nnz) {
  return lv_layout(std::min<int64_t>(std::max<int64_t>(n, 0), LV_MAX_N), std::min<int64_t>(std::max<int64_t>(nnz, 0), LV_MAX_NNZ)).total;
}

int launch_louvain_device(int64_t n, const int64_t *d_ptr, const int32_t *d_adj, const uint16_t *d_codes, const uint16_t *d_loops, const double *values,
                          int n_values, double resolution, uint32_t seed, void *d_work, size_t work_bytes, int32_t *d_membership, double *modularity_out,
                          int32_t *levels_out, int32_t *iterations_out, hipStream_t stream) {
  if (n > LV_MAX_N) return fail(DA_ERR_UNSUPPORTED, "device Louvain: too many vertices");
  // the weight table, on the host: wq[code] = rint(values[code] * 2^30)
  std::vector<long long> wq((size_t)std::max(n_values, 1), 0);
  long long wq_max = 0;
  for (int c = 0; c < n_values; ++c) {
    const double v = values[c];
    if (!std::isfinite(v) || v < 0.0) return fail(DA_ERR_BAD_ARG, "device Louvain: weights must be finite and not negative (values[%d])", c);
    const double scaled = std::nearbyint(v * 1073741824.0);
    if (scaled >= 4611686018427387904.0) return fail(DA_ERR_UNSUPPORTED, "device Louvain: weight too large (values[%d])", c);
    wq[(size_t)c] = (long long)scaled;
    wq_max = std::max(wq_max, wq[(size_t)c]);
  }
  long long ends[2] = {0, 0};
  DA_HIP_TRY(hipMemcpyAsync(&ends[0], d_ptr, 8, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipMemcpyAsync(&ends[1], d_ptr + n, 8, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipStreamSynchronize(stream));
  const long long nnz = ends[1];
  if (ends[0] != 0 || nnz < 0) return fail(DA_ERR_BAD_ARG, "device Louvain: row pointers must start at 0 and not decrease");
  if (nnz > LV_MAX_NNZ) return fail(DA_ERR_UNSUPPORTED, "device Louvain: more than %lld adjacency entries", (long long)LV_MAX_NNZ);
  if (nnz > 0 && (!d_adj || !d_codes)) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  if ((unsigned __int128)((unsigned long long)nnz + 2ull * (unsigned long long)n) * (unsigned __int128)(unsigned long long)wq_max >=
      ((unsigned __int128)1 << 62))
    return fail(DA_ERR_UNSUPPORTED, "device Louvain: total weight could reach 2^62");
  const LvLayout L = lv_layout(n, nnz);
  if (work_bytes < L.total) return fail(DA_ERR_BAD_ARG, "device Louvain: workspace too small (%zu < %zu bytes)", work_bytes, L.total);
  char *work = static_cast<char *>(d_work);
  LvRecord *d_rec = at_bytes<LvRecord>(work, L.rec);
  // k_lv_validate: nothing below runs on a graph that fails it
  unsigned bad = 0;
  DA_HIP_TRY(hipMemsetAsync(d_rec, 0, sizeof(LvRecord), stream));
  hipLaunchKernelGGL(k_lv_validate, dim3(lv_blocks(n, LV_WAVES)), dim3(LV_THREADS), 0, stream, reinterpret_cast<const long long *>(d_ptr), d_adj, d_codes,
                     d_loops, n, nnz, n_values, &d_rec->bad);
  DA_HIP_TRY(hipGetLastError());
  DA_HIP_TRY(hipMemcpyAsync(&bad, &d_rec->bad, 4, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipStreamSynchronize(stream));
  if (bad) return fail(DA_ERR_BAD_ARG, "device Louvain: the CSR is not canonical (row pointers, neighbour order or range, a diagonal entry, or a code >= n_values)");
  long long *d_wq = at_bytes<long long>(work, L.wq);
  DA_HIP_TRY(hipMemcpyAsync(d_wq, wq.data(), wq.size() * 8, hipMemcpyHostToDevice, stream));
  int32_t *d_member = at_bytes<int32_t>(work, L.member);
  hipLaunchKernelGGL(k_lv_iota, dim3(lv_blocks(n, LV_THREADS)), dim3(LV_THREADS), 0, stream, d_member, n);
  DA_HIP_TRY(hipGetLastError());

  LvGraph g;
  g.ptr = reinterpret_cast<const long long *>(d_ptr); g.adj = d_adj; g.codes = d_codes; g.wq = d_wq; g.w = nullptr;
  long long *d_loop = at_bytes<long long>(work, L.loop0);
  int64_t n_level = n, nnz_level = nnz;
  int levels = 0, rc;
  double q = 0.0;
  unsigned long long m2 = 0;
  for (int level = 0; level < LV_MAX_LEVELS; ++level) {
    bool moved = false;
    int its = 0;
    unsigned long long m2_level = 0;
    rc = level == 0 ? lv_level<true>(g, d_loops, d_loop, n_level, level, seed, resolution, work, L, m2, &moved, &its, &q, &m2_level, stream)
                    : lv_level<false>(g, nullptr, d_loop, n_level, level, seed, resolution, work, L, m2, &moved, &its, &q, &m2_level, stream);
    if (rc != DA_OK) return rc;
    if (level == 0) {
      m2 = m2_level;
      if (m2 == 0) { q = 0.0; break; }
    }
    if (iterations_out) iterations_out[levels] = its;
    ++levels;
    if (!moved) break;
    const bool to_a = (level & 1) == 0;
    long long *n_ptr = at_bytes<long long>(work, to_a ? L.ptr_a : L.ptr_b), *n_w = at_bytes<long long>(work, to_a ? L.w_a : L.w_b);
    long long *n_loop = at_bytes<long long>(work, to_a ? L.loop_a : L.loop_b);
    int32_t *n_adj = at_bytes<int32_t>(work, to_a ? L.adj_a : L.adj_b);
    int64_t nc = 0, nnz_next = 0;
    rc = level == 0 ? lv_aggregate<true>(g, d_loop, n_level, n, nnz, work, L, n_ptr, n_adj, n_w, n_loop, &nc, &nnz_next, stream)
                    : lv_aggregate<false>(g, d_loop, n_level, n, nnz, work, L, n_ptr, n_adj, n_w, n_loop, &nc, &nnz_next, stream);
    if (rc != DA_OK) return rc;
    const bool merged = nc < n_level;
    g.ptr = n_ptr; g.adj = n_adj; g.codes = nullptr; g.wq = nullptr; g.w = n_w;
    d_loop = n_loop;
    n_level = nc;
    nnz_level = nnz_next;
    if (!merged) break;
  }
  (void)nnz_level;
  // ids from 1 in order of first appearance by vertex
  std::vector<int32_t> member((size_t)n), rank((size_t)n, 0);
  DA_HIP_TRY(hipMemcpyAsync(member.data(), d_member, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipStreamSynchronize(stream));
  int32_t next_id = 0;
  for (int64_t v = 0; v < n; ++v) {
    const int32_t c = member[(size_t)v];
    if (c < 0 || c >= n) return fail(DA_ERR_HIP, "device Louvain: membership out of range (internal error)");
    if (rank[(size_t)c] == 0) rank[(size_t)c] = ++next_id;
    member[(size_t)v] = rank[(size_t)c];
  }
  DA_HIP_TRY(hipMemcpyAsync(d_membership, member.data(), (size_t)n * 4, hipMemcpyHostToDevice, stream));
  DA_HIP_TRY(hipStreamSynchronize(stream));
  if (modularity_out) *modularity_out = q;
  if (levels_out) *levels_out = levels;
  return DA_OK;
}

}  // namespace da
