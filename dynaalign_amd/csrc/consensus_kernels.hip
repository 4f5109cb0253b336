// consensus_kernels.hip -- the center-star consensus of clusters on the device (da_dev_cluster_consensus and its pieces).
//
// The clusters are a POOLED table: members of cluster k are the sequences cluster_ptr[k] .. cluster_ptr[k + 1] - 1, c_k of them.  Two
// numberings follow from it and nothing else is ever listed on the host:
//   * PAIRS (phase 1): all ordered pairs of a cluster, i ascending then j != i ascending; cluster k owns pair_ptr[k] .. pair_ptr[k + 1] - 1,
//     pair_ptr the running sum of c (c - 1) (int64: one cluster of 10^5 members is 10^10 pairs), member i of it the c - 1 consecutive
//     pairs from pair_ptr[k] + i (c - 1);
//   * ROWS (phase 2): (center, j != center), j ascending; cluster k owns rows cluster_ptr[k] - k .. cluster_ptr[k + 1] - (k + 1) - 1.
//
//   k_cons_pair_ptr     pair_ptr from cluster_ptr (one workgroup)
//   k_cons_pairs        (pair_x, pair_y) of a range of pairs or rows: what da_dev_nw_align[_long]_pairs reads
//   k_cons_center_sums  a wave per member: the sum of matches / length over the member's pairs inside the block, as 63-bit fixed point
//                       in two 64-bit limbs, ADDED to the member's limbs.  The double matches / length (the device's IEEE divide, as in
//                       the similarity kernels) times 2^63 is an integer below 2^64 for every length up to 2048, so the limbs hold the
//                       EXACT sum whatever the order.  Blocks may be cut anywhere; a member is owned by one wave per launch and
//                       launches are ordered on the stream, so there are no atomics.
//   k_cons_pick         a wave per cluster: every member's sum rounded to 53 significant bits, ties to even -- what math.fsum returns --
//                       then the largest, the lowest index among equals
//   k_cons_vote         a workgroup per cluster: the tally [position][25] as uint32 in LDS, a wave per ops row, 64 ops at a time; a
//                       lane's center position and member position are the popcounts of the D|U and D|L lanes below it plus a running
//                       base; LDS integer adds (order-free, so deterministic); a last pass applies the tie rule and compacts out the
//                       columns '-' wins.  Centers longer than the window are walked once per window of CN_WINDOW positions.
#include "da_common.hpp"

namespace da {
namespace {

constexpr int CN_THREADS = 256;
constexpr int CN_WAVES = CN_THREADS / 64;
constexpr int CN_SYMS = 25;          // codes 0 .. 23 of da_dev_nw_encode and the gap, 24
constexpr int CN_GAP = 24;
constexpr int CN_WINDOW = 512;       // tally positions held at once: 50 KiB of LDS
constexpr int CN_WINDOW_SHORT = 128; // ... when no center has more than 128 residues: 12.5 KiB
constexpr int64_t CN_BLOCK_CAP = (int64_t)1 << 20;   // pairs or rows of one block

template <typename T> __device__ __forceinline__ T cn_min(T a, T b) { return a < b ? a : b; }
template <typename T> __device__ __forceinline__ T cn_max(T a, T b) { return a > b ? a : b; }

// the largest k in [0, count) with ptr[k] - k * sub <= v; ptr has count + 1 entries and ptr[0] <= v.  With equal keys (clusters that own
// nothing) this is the last of them, the one that owns v.
__device__ __forceinline__ int64_t cn_find(const int64_t *__restrict__ ptr, int64_t count, int64_t v, int64_t sub) {
  int64_t lo = 0, hi = count;
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (ptr[mid] - mid * sub <= v) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(1024) void k_cons_pair_ptr(const int64_t *__restrict__ cluster_ptr, int64_t clusters, int64_t *__restrict__ pair_ptr) {
  __shared__ int64_t part[1024];
  const int64_t chunk = (clusters + 1023) / 1024;
  const int64_t k0 = cn_min<int64_t>((int64_t)threadIdx.x * chunk, clusters), k1 = cn_min<int64_t>(k0 + chunk, clusters);
  int64_t s = 0;
  for (int64_t k = k0; k < k1; ++k) {
    const int64_t c = cluster_ptr[k + 1] - cluster_ptr[k];
    s += c * (c - 1);
  }
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t run = 0;
    for (int t = 0; t < 1024; ++t) { const int64_t v = part[t]; part[t] = run; run += v; }
    pair_ptr[clusters] = run;
  }
  __syncthreads();
  s = part[threadIdx.x];
  for (int64_t k = k0; k < k1; ++k) {
    const int64_t c = cluster_ptr[k + 1] - cluster_ptr[k];
    pair_ptr[k] = s;
    s += c * (c - 1);
  }
}

// entries [p0, p1) of a numbering into pair_x / pair_y[p - p0].  center == NULL: the pairs; otherwise the rows.
__global__ __launch_bounds__(CN_THREADS) void k_cons_pairs(const int64_t *__restrict__ cluster_ptr, const int64_t *__restrict__ pair_ptr,
                                                           int64_t clusters, const int32_t *__restrict__ center, int64_t p0, int64_t p1,
                                                           int32_t *__restrict__ pair_x, int32_t *__restrict__ pair_y) {
  const int64_t p = p0 + (int64_t)blockIdx.x * CN_THREADS + threadIdx.x;
  if (p >= p1) return;
  if (!center) {
    const int64_t k = cn_find(pair_ptr, clusters, p, 0);
    const int64_t b = cluster_ptr[k], c = cluster_ptr[k + 1] - b, r = p - pair_ptr[k];
    const int64_t i = r / (c - 1), jj = r - i * (c - 1);
    pair_x[p - p0] = (int32_t)(b + i);
    pair_y[p - p0] = (int32_t)(b + jj + (jj >= i ? 1 : 0));
  } else {
    const int64_t k = cn_find(cluster_ptr, clusters, p, 1);
    const int64_t b = cluster_ptr[k], r = p - (b - k), cen = (int64_t)center[k] - b;
    pair_x[p - p0] = center[k];
    pair_y[p - p0] = (int32_t)(b + r + (r >= cen ? 1 : 0));
  }
}

// len / matches: the results of pairs [p0, p1), entry p - p0.  Wave w owns member g0 + w (g1: one past the last member the block touches).
__global__ __launch_bounds__(CN_THREADS) void k_cons_center_sums(const int32_t *__restrict__ len, const int32_t *__restrict__ matches, int64_t p0,
                                                                 int64_t p1, const int64_t *__restrict__ cluster_ptr,
                                                                 const int64_t *__restrict__ pair_ptr, int64_t clusters, int64_t g0, int64_t g1,
                                                                 uint64_t *__restrict__ sums) {
  const int lane = threadIdx.x & 63;
  const int64_t g = g0 + (int64_t)blockIdx.x * CN_WAVES + (threadIdx.x >> 6);
  if (g >= g1) return;
  const int64_t k = cn_find(cluster_ptr, clusters, g, 0);
  const int64_t b = cluster_ptr[k], c = cluster_ptr[k + 1] - b;
  const int64_t first = pair_ptr[k] + (g - b) * (c - 1);
  const int64_t lo_p = cn_max(first, p0), hi_p = cn_min(first + (c - 1), p1);
  uint64_t lo = 0, hi = 0;
  for (int64_t t = lo_p + lane; t < hi_p; t += 64) {
    const int32_t l = len[t - p0], m = matches[t - p0];
    if (l > 0 && m > 0) {                                   // a pair of two empty strings counts 0.0
      const double q = (double)m / (double)l;               // the divide of the similarity kernels
      const uint64_t term = (uint64_t)(q * 9223372036854775808.0);   // * 2^63: exact, and an integer (see above)
      lo += term;
      hi += lo < term ? 1u : 0u;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint64_t olo = __shfl_down((unsigned long long)lo, off, 64), ohi = __shfl_down((unsigned long long)hi, off, 64);
    lo += olo;
    hi += ohi + (lo < olo ? 1u : 0u);
  }
  if (lane == 0 && hi_p > lo_p) {
    const uint64_t slo = sums[2 * g], shi = sums[2 * g + 1];
    const uint64_t nlo = slo + lo;
    sums[2 * g] = nlo;
    sums[2 * g + 1] = shi + hi + (nlo < slo ? 1u : 0u);
  }
}

// the 128-bit integer (hi, lo) rounded to 53 significant bits, ties to even: the double the exact sum rounds to, still as an integer
__device__ __forceinline__ void cn_round53(uint64_t &hi, uint64_t &lo) {
  const int top = hi ? 127 - __clzll((long long)hi) : (lo ? 63 - __clzll((long long)lo) : -1);
  if (top < 53) return;
  const int drop = top - 52;                                // 1 .. 75 low bits go
  unsigned __int128 v = ((unsigned __int128)hi << 64) | lo;
  const unsigned __int128 half = (unsigned __int128)1 << (drop - 1);
  const unsigned __int128 rem = v & ((half << 1) - 1);
  v >>= drop;
  if (rem > half || (rem == half && ((uint64_t)v & 1u))) ++v;
  v <<= drop;
  hi = (uint64_t)(v >> 64);
  lo = (uint64_t)v;
}

__global__ __launch_bounds__(CN_THREADS) void k_cons_pick(const uint64_t *__restrict__ sums, const int64_t *__restrict__ cluster_ptr, int64_t clusters,
                                                          int32_t *__restrict__ center) {
  const int lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * CN_WAVES + (threadIdx.x >> 6);
  if (k >= clusters) return;
  const int64_t b = cluster_ptr[k], c = cluster_ptr[k + 1] - b;
  uint64_t bhi = 0, blo = 0;
  int64_t bi = INT64_MAX;
  for (int64_t i = lane; i < c; i += 64) {
    uint64_t lo = sums[2 * (b + i)], hi = sums[2 * (b + i) + 1];
    cn_round53(hi, lo);
    if (bi == INT64_MAX || hi > bhi || (hi == bhi && lo > blo)) { bhi = hi; blo = lo; bi = i; }   // strictly larger: the lowest index stays
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint64_t ohi = __shfl_xor((unsigned long long)bhi, off, 64), olo = __shfl_xor((unsigned long long)blo, off, 64);
    const int64_t oi = __shfl_xor((long long)bi, off, 64);
    const bool other_valid = oi != INT64_MAX, mine_valid = bi != INT64_MAX;
    const bool larger = ohi > bhi || (ohi == bhi && olo > blo), equal = ohi == bhi && olo == blo;
    if (other_valid && (!mine_valid || larger || (equal && oi < bi))) { bhi = ohi; blo = olo; bi = oi; }
  }
  if (lane == 0) center[k] = (int32_t)(b + (bi == INT64_MAX ? 0 : bi));
}

// ops: the rows [q_lo, q_hi) of the row numbering, row q at ops + (q - q_lo) * ld_ops, its length at len[q - q_lo] (len == NULL: the row
// ends at its first 0 byte or at ld_ops).  Workgroup x does cluster k0 + x.  A cluster whose rows are all inside [q_lo, q_hi) is tallied
// and written out; one that starts before q_lo takes its tally from `carry` first, one that goes on past q_hi leaves it there and writes
// nothing -- so a cluster too large for one block is done in consecutive launches over [k, k + 1).
template <int W>
__global__ __launch_bounds__(CN_THREADS) void k_cons_vote(const uint8_t *__restrict__ codes, const int64_t *__restrict__ offsets,
                                                          const int64_t *__restrict__ cluster_ptr, const int32_t *__restrict__ center, int64_t k0,
                                                          const uint8_t *__restrict__ ops, int64_t ld_ops, const int32_t *__restrict__ len,
                                                          int64_t q_lo, int64_t q_hi, uint32_t *__restrict__ carry, uint8_t *__restrict__ cons,
                                                          int64_t ld_cons, int32_t *__restrict__ cons_len) {
  __shared__ uint32_t tally[W * CN_SYMS];
  __shared__ int wave_kept[CN_WAVES];
  __shared__ int out_base;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t k = k0 + blockIdx.x;
  const int64_t b = cluster_ptr[k], c = cluster_ptr[k + 1] - b;
  const int64_t vb = b - k, ve = vb + c - 1;                 // the cluster's rows
  const int64_t r_lo = cn_max(vb, q_lo), r_hi = cn_min(ve, q_hi);
  const bool first = q_lo <= vb, last = q_hi >= ve;
  const int64_t cen_g = center[k];
  const int64_t cen_at = offsets[cen_g];
  const int L = (int)(offsets[cen_g + 1] - cen_at);
  const uint8_t *cen = codes + cen_at;
  const int64_t cen_local = cen_g - b;
  const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  if (tid == 0) out_base = 0;
  __syncthreads();
  for (int w0 = 0; w0 < L; w0 += W) {
    const int wl = cn_min(W, L - w0);
    for (int e = tid; e < wl * CN_SYMS; e += CN_THREADS) tally[e] = first ? 0u : carry[(size_t)w0 * CN_SYMS + e];
    __syncthreads();
    if (first)
      for (int p = tid; p < wl; p += CN_THREADS) {
        const uint32_t s = cen[w0 + p];
        if (s < CN_SYMS) tally[p * CN_SYMS + s] = 1u;       // the center's own residue
      }
    __syncthreads();
    for (int64_t r = r_lo + wave; r < r_hi; r += CN_WAVES) {
      const uint8_t *row = ops + (size_t)(r - q_lo) * (size_t)ld_ops;
      const int64_t jl = r - vb, mem_g = b + jl + (jl >= cen_local ? 1 : 0);
      const int64_t mem_at = offsets[mem_g];
      const int ML = (int)(offsets[mem_g + 1] - mem_at);
      const uint8_t *mem = codes + mem_at;
      int n_ops = (int)ld_ops;
      if (len) n_ops = cn_max(0, cn_min(n_ops, (int)len[r - q_lo]));
      int pbase = 0, qbase = 0;
      for (int t = 0; t < n_ops && pbase < w0 + wl; t += 64) {
        const int at = t + lane;
        const uint8_t op = at < n_ops ? row[at] : (uint8_t)0;
        const bool isd = op == 'D', isu = op == 'U', isl = op == 'L';
        const uint64_t du = __ballot(isd || isu), dl = __ballot(isd || isl);
        const int p = pbase + __popcll(du & below), q = qbase + __popcll(dl & below);
        if ((isd || isu) && p >= w0 && p < w0 + wl) {
          uint32_t s = CN_GAP;
          if (isd) s = q < ML ? (uint32_t)mem[q] : (uint32_t)CN_SYMS;
          if (s < CN_SYMS) atomicAdd(&tally[(p - w0) * CN_SYMS + s], 1u);
        }
        pbase += __popcll(du);
        qbase += __popcll(dl);
        if (__ballot(at < n_ops && op == 0) != 0ull) break;   // the row ended inside this chunk
      }
    }
    __syncthreads();
    if (!last) {
      for (int e = tid; e < wl * CN_SYMS; e += CN_THREADS) carry[(size_t)w0 * CN_SYMS + e] = tally[e];
    } else {
      for (int base = 0; base < wl; base += CN_THREADS) {
        const int p = base + tid;
        bool keep = false;
        uint8_t letter = 0;
        if (p < wl) {
          const uint32_t *col = tally + p * CN_SYMS;
          uint32_t top = 0;
          int win = 0;
          for (int s = 0; s < CN_SYMS; ++s)
            if (col[s] > top) { top = col[s]; win = s; }     // the smallest code among the most frequent
          const uint32_t own = cen[w0 + p];
          if (own < CN_SYMS && col[own] == top) win = (int)own;   // ... unless the center's residue is one of them
          keep = win != CN_GAP;
          letter = (uint8_t)"ARNDCQEGHILKMFPSTWYVBZX*-"[win];
        }
        const uint64_t kept = __ballot(keep);
        if (lane == 0) wave_kept[wave] = __popcll(kept);
        __syncthreads();
        int at = out_base + __popcll(kept & below);
        for (int w = 0; w < wave; ++w) at += wave_kept[w];
        if (keep && at < ld_cons) cons[(size_t)k * (size_t)ld_cons + at] = letter;
        __syncthreads();
        if (tid == 0) {
          int total = 0;
          for (int w = 0; w < CN_WAVES; ++w) total += wave_kept[w];
          out_base += total;
        }
        __syncthreads();
      }
    }
    __syncthreads();
  }
  if (last && tid == 0) cons_len[k] = out_base;
}

inline size_t cn_align_up(size_t v) { return (v + 255) / 256 * 256; }

// the call's workspace: [sums | pair_ptr | carry | the running phase: pair_x | pair_y | len | matches | ops rows (phase 2) | alignment workspace]
struct ConsPhase { size_t px, py, len, mt, ops, work, work_bytes, end; int64_t cap; };
struct ConsPlan {
  size_t sums, pair_ptr, carry, total;
  ConsPhase ph[2];                 // 0: blocks of pairs (phase 1), 1: blocks of rows (phase 2)
  int64_t ld_ops;
  bool is_long;
};

// work_bytes == 0: the sizes at which the phases take blocks of want1 pairs / want2 rows; otherwise the largest blocks that fit.
bool cons_plan(int64_t n, int64_t clusters, int64_t max_len, int64_t want1, int64_t want2, size_t work_bytes, ConsPlan *pl) {
  pl->is_long = max_len > 127;
  pl->ld_ops = std::max<int64_t>(2 * max_len, 1);
  size_t at = 0;
  pl->sums = at; at += cn_align_up((size_t)std::max<int64_t>(n, 1) * 16);
  pl->pair_ptr = at; at += cn_align_up((size_t)(clusters + 1) * sizeof(int64_t));
  pl->carry = at; at += cn_align_up((size_t)CN_SYMS * (size_t)std::max<int64_t>(max_len, 1) * sizeof(uint32_t));
  const size_t fixed = at;
  int64_t want[2] = {std::min(std::max<int64_t>(ceil_div(want1, 64) * 64, 64), CN_BLOCK_CAP),
                     std::min(std::max<int64_t>(ceil_div(want2, 64) * 64, 64), CN_BLOCK_CAP)};
  const size_t short_pp = nw_align_workspace_bytes(64) / 64;          // the lane-per-pair kernels' bytes per pair
  const size_t slot = pl->is_long ? nw_align_long_slot_bytes(max_len) : 0;
  int64_t slots = pl->is_long ? std::min<int64_t>(want[1], 3072) : 0;  // the wavefront kernel keeps decisions only with ops: phase 2
  const size_t per[2] = {16 + (pl->is_long ? 0 : short_pp), 16 + (size_t)pl->ld_ops + (pl->is_long ? 0 : short_pp)};
  if (work_bytes != 0) {
    if (work_bytes <= fixed) return false;
    const size_t avail = work_bytes - fixed;
    if (pl->is_long) slots = std::max<int64_t>(1, std::min<int64_t>(slots, (int64_t)(avail / 2 / slot)));
    for (int f = 0; f < 2; ++f) {
      const size_t held = f == 1 ? (size_t)slots * slot : 0;
      if (avail < held) return false;
      want[f] = std::min<int64_t>(want[f], (int64_t)((avail - held) / per[f]) / 64 * 64);
      if (want[f] < 64) return false;
    }
  }
  pl->total = fixed;
  for (int f = 0; f < 2; ++f) {
    ConsPhase &ph = pl->ph[f];
    ph.cap = want[f];
    const size_t ints = (size_t)ph.cap * sizeof(int32_t);            // a multiple of 256
    ph.px = fixed; ph.py = ph.px + ints; ph.len = ph.py + ints; ph.mt = ph.len + ints; ph.ops = ph.mt + ints;
    ph.work = ph.ops + (f == 1 ? (size_t)ph.cap * (size_t)pl->ld_ops : 0);
    ph.work_bytes = pl->is_long ? (f == 1 ? (size_t)slots * slot : 0) : nw_align_workspace_bytes(ph.cap);
    ph.end = ph.work + ph.work_bytes;
    pl->total = std::max(pl->total, ph.end);
  }
  return work_bytes == 0 || pl->total <= work_bytes;
}

int cn_align(const ConsPlan &pl, uint8_t *w, int f, const uint8_t *d_codes, const int64_t *d_off, int64_t n, int64_t cnt, int64_t max_len, int mid,
             int go, int ge, hipStream_t stream) {
  const ConsPhase &ph = pl.ph[f];
  int32_t *px = reinterpret_cast<int32_t *>(w + ph.px), *py = reinterpret_cast<int32_t *>(w + ph.py);
  int32_t *ln = reinterpret_cast<int32_t *>(w + ph.len), *mt = reinterpret_cast<int32_t *>(w + ph.mt);
  uint8_t *ops = f == 1 ? w + ph.ops : nullptr;
  if (pl.is_long)
    return launch_nw_align_long(d_codes, d_off, n, d_codes, d_off, n, px, py, 0, cnt, mid, go, ge, ops, pl.ld_ops, ln, mt, nullptr, max_len,
                                ph.work_bytes ? w + ph.work : nullptr, ph.work_bytes, stream);
  return launch_nw_align(d_codes, d_off, n, d_codes, d_off, n, px, py, 0, cnt, mid, go, ge, ops, pl.ld_ops, ln, mt, nullptr, w + ph.work,
                         ph.work_bytes, stream);
}

// sum of c (c - 1) and of c - 1 over the clusters, from the host copy of cluster_ptr
void cn_totals(const int64_t *cluster_ptr, int64_t clusters, int64_t *pairs, int64_t *rows) {
  int64_t p = 0;
  for (int64_t k = 0; k < clusters; ++k) {
    const int64_t c = cluster_ptr[k + 1] - cluster_ptr[k];
    p += c * (c - 1);
  }
  *pairs = p;
  *rows = cluster_ptr[clusters] - cluster_ptr[0] - clusters;
}

}  // namespace

int launch_cons_pair_ptr(const int64_t *d_cluster_ptr, int64_t clusters, int64_t *d_pair_ptr, hipStream_t stream) {
  hipLaunchKernelGGL(k_cons_pair_ptr, dim3(1), dim3(1024), 0, stream, d_cluster_ptr, clusters, d_pair_ptr);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

int launch_cons_pairs(const int64_t *d_cluster_ptr, const int64_t *d_pair_ptr, int64_t clusters, const int32_t *d_center, int64_t p0, int64_t p1,
                      int32_t *d_pair_x, int32_t *d_pair_y, hipStream_t stream) {
  if (p1 <= p0) return DA_OK;
  hipLaunchKernelGGL(k_cons_pairs, dim3((unsigned)ceil_div(p1 - p0, CN_THREADS)), dim3(CN_THREADS), 0, stream, d_cluster_ptr, d_pair_ptr, clusters,
                     d_center, p0, p1, d_pair_x, d_pair_y);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

// The members a block of pairs [p0, p1) touches are found on the host copy of the table (pair_ptr_host: its running sums of c (c - 1)).
int launch_cons_center_sums(const int32_t *d_len, const int32_t *d_matches, int64_t p0, int64_t p1, const int64_t *cluster_ptr_host,
                            const int64_t *pair_ptr_host, const int64_t *d_cluster_ptr, const int64_t *d_pair_ptr, int64_t clusters, uint64_t *d_sums,
                            hipStream_t stream) {
  if (p1 <= p0) return DA_OK;
  auto member_of = [&](int64_t p) {
    const int64_t k = (std::upper_bound(pair_ptr_host, pair_ptr_host + clusters + 1, p) - pair_ptr_host) - 1;
    const int64_t c = cluster_ptr_host[k + 1] - cluster_ptr_host[k];
    return cluster_ptr_host[k] + (p - pair_ptr_host[k]) / (c - 1);
  };
  const int64_t g0 = member_of(p0), g1 = member_of(p1 - 1) + 1;
  hipLaunchKernelGGL(k_cons_center_sums, dim3((unsigned)ceil_div(g1 - g0, CN_WAVES)), dim3(CN_THREADS), 0, stream, d_len, d_matches, p0, p1,
                     d_cluster_ptr, d_pair_ptr, clusters, g0, g1, d_sums);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

int launch_cons_pick(const uint64_t *d_sums, const int64_t *d_cluster_ptr, int64_t clusters, int32_t *d_center, hipStream_t stream) {
  if (clusters <= 0) return DA_OK;
  hipLaunchKernelGGL(k_cons_pick, dim3((unsigned)ceil_div(clusters, CN_WAVES)), dim3(CN_THREADS), 0, stream, d_sums, d_cluster_ptr, clusters, d_center);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

int launch_cons_vote(const uint8_t *d_codes, const int64_t *d_off, const int64_t *d_cluster_ptr, const int32_t *d_center, int64_t k0, int64_t kcount,
                     const uint8_t *d_ops, int64_t ld_ops, const int32_t *d_len, int64_t q_lo, int64_t q_hi, uint32_t *d_carry, uint8_t *d_cons,
                     int64_t ld_cons, int32_t *d_cons_len, int64_t max_len, hipStream_t stream) {
  if (kcount <= 0) return DA_OK;
  if (max_len <= CN_WINDOW_SHORT)
    hipLaunchKernelGGL(k_cons_vote<CN_WINDOW_SHORT>, dim3((unsigned)kcount), dim3(CN_THREADS), 0, stream, d_codes, d_off, d_cluster_ptr, d_center, k0,
                       d_ops, ld_ops, d_len, q_lo, q_hi, d_carry, d_cons, ld_cons, d_cons_len);
  else
    hipLaunchKernelGGL(k_cons_vote<CN_WINDOW>, dim3((unsigned)kcount), dim3(CN_THREADS), 0, stream, d_codes, d_off, d_cluster_ptr, d_center, k0, d_ops,
                       ld_ops, d_len, q_lo, q_hi, d_carry, d_cons, ld_cons, d_cons_len);
  DA_HIP_TRY(hipGetLastError());
  return DA_OK;
}

// minimal: with blocks of 64 pairs / rows, the least the call takes; otherwise with the largest blocks it would use
size_t cluster_consensus_workspace_bytes(const int64_t *cluster_ptr_host, int64_t clusters, int64_t max_len, bool minimal) {
  if (!cluster_ptr_host || clusters <= 0 || max_len < 0) return 0;
  int64_t pairs, rows;
  cn_totals(cluster_ptr_host, clusters, &pairs, &rows);
  if (minimal) pairs = rows = 64;
  ConsPlan pl;
  cons_plan(cluster_ptr_host[clusters], clusters, std::min<int64_t>(max_len, 1024), pairs, rows, 0, &pl);
  return pl.total;
}

// Both phases, nothing returning to the host in between.  The blocks are planned on the host copy of the table; what the device reads is
// d_cluster_ptr.  Every cluster has at least one member (checked by the caller).
int launch_cluster_consensus(const uint8_t *d_codes, const int64_t *d_off, int64_t n, const int64_t *cluster_ptr_host, const int64_t *d_cluster_ptr,
                             int64_t clusters, int64_t max_len, int matrix_id, int gap_open, int gap_ext, uint8_t *d_cons, int64_t ld_cons,
                             int32_t *d_cons_len, int32_t *d_center, void *d_work, size_t work_bytes, hipStream_t stream) {
  int64_t pairs, rows;
  cn_totals(cluster_ptr_host, clusters, &pairs, &rows);
  ConsPlan pl;
  if (!cons_plan(n, clusters, max_len, pairs, rows, work_bytes, &pl))
    return fail(DA_ERR_BAD_ARG, "the consensus workspace is too small for blocks of 64 pairs (%zu bytes; da_dev_cluster_consensus_workspace_bytes)",
                work_bytes);
  uint8_t *w = static_cast<uint8_t *>(d_work);
  uint64_t *sums = reinterpret_cast<uint64_t *>(w + pl.sums);
  int64_t *d_pair_ptr = reinterpret_cast<int64_t *>(w + pl.pair_ptr);
  uint32_t *carry = reinterpret_cast<uint32_t *>(w + pl.carry);
  const ConsPhase &p1f = pl.ph[0], &p2f = pl.ph[1];
  std::vector<int64_t> pp((size_t)clusters + 1);
  pp[0] = 0;
  for (int64_t k = 0; k < clusters; ++k) {
    const int64_t c = cluster_ptr_host[k + 1] - cluster_ptr_host[k];
    pp[(size_t)k + 1] = pp[(size_t)k] + c * (c - 1);
  }
  int rc;
  DA_HIP_TRY(hipMemsetAsync(sums, 0, (size_t)std::max<int64_t>(n, 1) * 16, stream));
  if ((rc = launch_cons_pair_ptr(d_cluster_ptr, clusters, d_pair_ptr, stream)) != DA_OK) return rc;
  // phase 1: the centers.  Blocks of pairs, cut anywhere.
  for (int64_t p0 = 0; p0 < pairs; p0 += p1f.cap) {
    const int64_t p1 = std::min(pairs, p0 + p1f.cap);
    if ((rc = launch_cons_pairs(d_cluster_ptr, d_pair_ptr, clusters, nullptr, p0, p1, reinterpret_cast<int32_t *>(w + p1f.px),
                                reinterpret_cast<int32_t *>(w + p1f.py), stream)) != DA_OK) return rc;
    if ((rc = cn_align(pl, w, 0, d_codes, d_off, n, p1 - p0, max_len, matrix_id, gap_open, gap_ext, stream)) != DA_OK) return rc;
    if ((rc = launch_cons_center_sums(reinterpret_cast<int32_t *>(w + p1f.len), reinterpret_cast<int32_t *>(w + p1f.mt), p0, p1, cluster_ptr_host, pp.data(), d_cluster_ptr, d_pair_ptr, clusters, sums, stream)) != DA_OK) return rc;
  }
  if ((rc = launch_cons_pick(sums, d_cluster_ptr, clusters, d_center, stream)) != DA_OK) return rc;
  // phase 2: the votes.  Groups of whole clusters; a cluster with more rows than a block holds goes alone, in member chunks.
  auto row0 = [&](int64_t k) { return cluster_ptr_host[k] - cluster_ptr_host[0] - k; };
  auto block = [&](int64_t k0, int64_t kcount, int64_t q_lo, int64_t q_hi) {
    int r = DA_OK;
    if (q_hi > q_lo) {
      if ((r = launch_cons_pairs(d_cluster_ptr, d_pair_ptr, clusters, d_center, q_lo, q_hi, reinterpret_cast<int32_t *>(w + p2f.px),
                                 reinterpret_cast<int32_t *>(w + p2f.py), stream)) != DA_OK) return r;
      if ((r = cn_align(pl, w, 1, d_codes, d_off, n, q_hi - q_lo, max_len, matrix_id, gap_open, gap_ext, stream)) != DA_OK) return r;
    }
    return launch_cons_vote(d_codes, d_off, d_cluster_ptr, d_center, k0, kcount, w + p2f.ops, pl.ld_ops, reinterpret_cast<int32_t *>(w + p2f.len), q_lo, q_hi, carry, d_cons, ld_cons,
                            d_cons_len, max_len, stream);
  };
  for (int64_t k0 = 0; k0 < clusters;) {
    int64_t k1 = k0 + 1;
    while (k1 < clusters && row0(k1 + 1) - row0(k0) <= p2f.cap) ++k1;
    if (row0(k1) - row0(k0) <= p2f.cap) {
      if ((rc = block(k0, k1 - k0, row0(k0), row0(k1))) != DA_OK) return rc;
    } else {
      for (int64_t q = row0(k0); q < row0(k1); q += p2f.cap)
        if ((rc = block(k0, 1, q, std::min(row0(k1), q + p2f.cap))) != DA_OK) return rc;
    }
    k0 = k1;
  }
  return DA_OK;
}

}  // namespace da
