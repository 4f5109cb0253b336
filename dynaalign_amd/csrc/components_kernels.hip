// components_kernels.hip -- connected components on the device (da_dev_components_edges, da_dev_components_csr, and the tail of
// da_dev_lsh_components): the definition is clusterbreak.components_dense, reproduced element for element.
//
//   1. k_cc_validate: before anything indexes by an endpoint, every listed endpoint is in [0, n) and (CSR) the row pointers do not decrease
//      and stay inside [0, nnz]; a violation is an argument error and nothing further is launched;
//   2. k_cc_init: parent[v] = v;
//   3. the union step of components_common.hpp over the edges -- k_cc_union_edges (an edge list, optionally cut at a code), k_cc_union_csr
//      (CSR rows: a wave per row of up to 64 entries, the workgroup for longer ones), or k_lsh_union (lsh_kernels.hip: the kept candidate
//      slots).  Lock-free, one launch, no host loop; the invariants there make the forest's roots the component minima whatever the order;
//   4. k_cc_compress: parent[v] = root(v); k_cc_flags marks the roots, one hipcub exclusive sum numbers them in vertex order -- the order of
//      the component minima, which is the order of first appearance -- and k_cc_label writes membership[v] = 1 + scan[root(v)] and, if
//      asked, counts the sizes with integer atomics (order-free in value).  scan[n] is the number of components.
#include "components_common.hpp"
#include "lsh_common.hpp"

namespace da {
namespace {

constexpr int CC_THREADS = 256;
constexpr int CC_WAVES = CC_THREADS / 64;
constexpr int CC_WAVE_MAX = 64;                // rows of up to 64 entries: a lane per entry
constexpr int64_t CC_MAX_N = 0x7ffffff0LL;     // 2^31 - 16: vertex ids and the scan's item count are 32-bit

// endpoints: a[0 .. m) and, if given, b[0 .. m) in [0, n).  Row pointers, if given: 0 <= ptr[v] <= ptr[v + 1] <= nnz for v < n (ptr[0] = 0 and
// ptr[n] = nnz were read by the host).
__global__ __launch_bounds__(CC_THREADS) void k_cc_validate(const int32_t *__restrict__ a, const int32_t *__restrict__ b, int64_t m,
                                                            const long long *__restrict__ ptr, int64_t n, long long nnz, unsigned *__restrict__ bad) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool wrong = false;
  for (int64_t e = t0; e < m; e += stride) {
    const int32_t x = a[e], y = b ? b[e] : 0;
    if (x < 0 || x >= n || y < 0 || y >= n) wrong = true;
  }
  if (ptr)
    for (int64_t v = t0; v < n; v += stride) {
      const long long p0 = ptr[v], p1 = ptr[v + 1];
      if (p0 < 0 || p1 < p0 || p1 > nnz) wrong = true;
    }
  if (__ballot(wrong) && (threadIdx.x & 63) == 0) atomicOr(bad, 1u);
}

__global__ __launch_bounds__(CC_THREADS) void k_cc_init(int32_t *__restrict__ parent, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += stride) parent[v] = (int32_t)v;
}

// code (if given): only the edges with code[e] >= min_code count -- one list cut at several thresholds
__global__ __launch_bounds__(CC_THREADS) void k_cc_union_edges(const int32_t *__restrict__ ei, const int32_t *__restrict__ ej,
                                                               const uint16_t *__restrict__ code, int min_code, int64_t m, int32_t *parent) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += stride) {
    if (code && (int)code[e] < min_code) continue;
    const int32_t a = ei[e], b = ej[e];
    if (a != b) cc_union(parent, a, b);
  }
}

// A workgroup takes CC_THREADS rows at a time.  Its waves first take the rows of up to CC_WAVE_MAX entries, a row per wave and an entry
// per lane, and list the longer rows in LDS; then the whole workgroup walks each listed row.  upper_only (the caller says the CSR holds
// both directions of every edge): only the entries with adj > row count, which halves the unions.
__global__ __launch_bounds__(CC_THREADS) void k_cc_union_csr(const long long *__restrict__ ptr, const int32_t *__restrict__ adj, int64_t n,
                                                             int upper_only, int32_t *parent) {
  __shared__ int long_rows[CC_THREADS];
  __shared__ unsigned int n_long_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t tiles = (n + CC_THREADS - 1) / CC_THREADS;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    if (tid == 0) n_long_s = 0;
    __syncthreads();
    for (int q = wave; q < CC_THREADS; q += CC_WAVES) {
      const int64_t r = tile * CC_THREADS + q;
      if (r >= n) break;                                    // wave-uniform
      const long long p0 = ptr[r], deg = ptr[r + 1] - p0;
      if (deg > CC_WAVE_MAX) {
        if (lane == 0) long_rows[atomicAdd(&n_long_s, 1u)] = q;
        continue;
      }
      if (lane < deg) {
        const int32_t a = adj[p0 + lane];
        if (upper_only ? a > r : a != r) cc_union(parent, (int32_t)r, a);
      }
    }
    __syncthreads();
    const int n_long = (int)n_long_s;
    for (int k = 0; k < n_long; ++k) {
      const int64_t r = tile * CC_THREADS + long_rows[k];
      const long long p0 = ptr[r], p1 = ptr[r + 1];
      for (long long e = p0 + tid; e < p1; e += CC_THREADS) {
        const int32_t a = adj[e];
        if (upper_only ? a > r : a != r) cc_union(parent, (int32_t)r, a);
      }
    }
    __syncthreads();                                        // the list and its counter are the next tile's
  }
}

// Runs after the last union (a kernel boundary): every root found is final.  A word another lane compresses meanwhile holds its old parent
// or its root, both fine for the walk.
__global__ __launch_bounds__(CC_THREADS) void k_cc_compress(int32_t *parent, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += stride) cc_store(parent + v, cc_find(parent, (int32_t)v));
}

// flag[v] = 1 for a root, flag[n] = 0 (so that the exclusive sum ends with the number of components)
__global__ __launch_bounds__(CC_THREADS) void k_cc_flags(const int32_t *__restrict__ parent, int64_t n, int32_t *__restrict__ flag) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v <= n; v += stride) flag[v] = v < n && parent[v] == (int32_t)v ? 1 : 0;
}

// membership[v] = 1 + scan[root(v)]; sizes[label - 1] += 1.  The vertices of a large component are mostly neighbours in a wave: the lanes
// that share the first active lane's label add once, the others each for themselves.
__global__ __launch_bounds__(CC_THREADS) void k_cc_label(const int32_t *__restrict__ parent, const int32_t *__restrict__ scan, int64_t n,
                                                         int32_t *__restrict__ membership, int32_t *__restrict__ sizes) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, rounds = (n + stride - 1) / stride;
  int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t it = 0; it < rounds; ++it, v += stride) {    // every lane makes every round: the ballots below are wave-wide
    const bool live = v < n;
    int32_t label = 0;
    if (live) {
      label = 1 + scan[parent[v]];
      membership[v] = label;
    }
    if (!sizes) continue;
    const unsigned long long active = __ballot(live);
    if (!active) continue;
    const int leader = __ffsll((long long)active) - 1;
    const int32_t first = __shfl(label, leader);
    const unsigned long long same = __ballot(live && label == first);
    if (lane == leader) atomicAdd(&sizes[first - 1], (int32_t)__popcll(same));
    else if (live && label != first) atomicAdd(&sizes[label - 1], 1);
  }
}

inline size_t scan_i32_bytes(int64_t items) {
  size_t t = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t, (const int32_t *)nullptr, (int32_t *)nullptr, (int)items, nullptr);
  return t;
}

// the workspace of n vertices, cut into its arrays
struct CcLayout {
  size_t parent, flag, scan, bad, temp, temp_bytes, bytes;
  explicit CcLayout(int64_t n) {
    const size_t t = (size_t)n;
    size_t at = 0;
    auto take = [&](size_t b) { const size_t o = at; at += up256(b); return o; };
    parent = take(t * 4);
    flag = take((t + 1) * 4);
    scan = take((t + 1) * 4);
    bad = take(16);
    temp_bytes = scan_i32_bytes(n + 1);
    temp = take(temp_bytes);
    bytes = at + 256;                                       // the arrays start on 256 bytes whatever the caller's pointer
  }
};

// grid-stride launches: 8 workgroups per CU at most (DYNAALIGN_CC_BLOCKS: another cap, for tests that want many passes at a small n)
inline unsigned cc_grid(int64_t items) { return (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div(items, CC_THREADS), 1), components_max_blocks()); }

int cc_check_work(int64_t n, const void *d_work, size_t work_bytes, const CcLayout &L) {
  if (n <= 0 || n > CC_MAX_N) return fail(DA_ERR_UNSUPPORTED, "components: n must be in 1 .. 2^31 - 16 (got %lld)", (long long)n);
  if (!d_work || work_bytes < L.bytes) return fail(DA_ERR_BAD_ARG, "components: workspace too small (%zu bytes, %zu needed)", work_bytes, L.bytes);
  return DA_OK;
}

// *bad_host = what k_cc_validate found; synchronises
int cc_validate(const int32_t *d_a, const int32_t *d_b, int64_t m, const int64_t *d_ptr, int64_t n, int64_t nnz, void *work, const CcLayout &L,
                unsigned *bad_host, hipStream_t stream) {
  unsigned *d_bad = at_bytes<unsigned>(work, L.bad);
  DA_HIP_TRY(hipMemsetAsync(d_bad, 0, 4, stream));
  hipLaunchKernelGGL(k_cc_validate, dim3(cc_grid(std::max(m, d_ptr ? n : 0))), dim3(CC_THREADS), 0, stream, d_a, d_b, m,
                     reinterpret_cast<const long long *>(d_ptr), n, (long long)nnz, d_bad);
  DA_HIP_TRY(hipGetLastError());
  DA_HIP_TRY(hipMemcpyAsync(bad_host, d_bad, 4, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipStreamSynchronize(stream));
  return DA_OK;
}

}  // namespace

int components_max_blocks() { return config().cc_blocks > 0 ? config().cc_blocks : 256 * 8; }

// sizes are asked for before anything is validated: n outside what the calls accept is clamped to their limits (the calls refuse it)
size_t components_workspace_bytes(int64_t n) { return CcLayout(std::min<int64_t>(std::max<int64_t>(n, 0), CC_MAX_N)).bytes; }

int launch_cc_init(int64_t n, void *d_work, size_t work_bytes, int32_t **d_parent_out, hipStream_t stream) {
  const CcLayout L(std::min<int64_t>(std::max<int64_t>(n, 0), CC_MAX_N));
  int rc;
  if ((rc = cc_check_work(n, d_work, work_bytes, L)) != DA_OK) return rc;
  int32_t *parent = at_bytes<int32_t>(align256(static_cast<char *>(d_work)), L.parent);
  hipLaunchKernelGGL(k_cc_init, dim3(cc_grid(n)), dim3(CC_THREADS), 0, stream, parent, n);
  DA_HIP_TRY(hipGetLastError());
  *d_parent_out = parent;
  return DA_OK;
}

int launch_cc_finish(int64_t n, void *d_work, size_t work_bytes, int32_t *d_membership, int32_t *d_sizes, int64_t *n_components_out,
                     hipStream_t stream) {
  const CcLayout L(std::min<int64_t>(std::max<int64_t>(n, 0), CC_MAX_N));
  int rc;
  if ((rc = cc_check_work(n, d_work, work_bytes, L)) != DA_OK) return rc;
  char *work = align256(static_cast<char *>(d_work));
  int32_t *parent = at_bytes<int32_t>(work, L.parent), *flag = at_bytes<int32_t>(work, L.flag), *scan = at_bytes<int32_t>(work, L.scan);
  const unsigned grid = cc_grid(n + 1);
  hipLaunchKernelGGL(k_cc_compress, dim3(grid), dim3(CC_THREADS), 0, stream, parent, n);
  DA_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_cc_flags, dim3(grid), dim3(CC_THREADS), 0, stream, parent, n, flag);
  DA_HIP_TRY(hipGetLastError());
  size_t tb = L.temp_bytes;
  DA_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(at_bytes<char>(work, L.temp), tb, flag, scan, (int)(n + 1), stream));
  if (d_sizes) DA_HIP_TRY(hipMemsetAsync(d_sizes, 0, (size_t)n * 4, stream));
  hipLaunchKernelGGL(k_cc_label, dim3(grid), dim3(CC_THREADS), 0, stream, parent, scan, n, d_membership, d_sizes);
  DA_HIP_TRY(hipGetLastError());
  int32_t count = 0;
  DA_HIP_TRY(hipMemcpyAsync(&count, scan + n, 4, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipStreamSynchronize(stream));
  *n_components_out = (int64_t)count;
  return DA_OK;
}

int launch_components_edges(const int32_t *d_i, const int32_t *d_j, const uint16_t *d_code, int min_code, int64_t m, int64_t n, void *d_work,
                            size_t work_bytes, int32_t *d_membership, int32_t *d_sizes, int64_t *n_components_out, hipStream_t stream) {
  const CcLayout L(std::min<int64_t>(std::max<int64_t>(n, 0), CC_MAX_N));
  int rc;
  if ((rc = cc_check_work(n, d_work, work_bytes, L)) != DA_OK) return rc;
  if (m > 0) {                                              // k_cc_validate: nothing below runs on a list that fails it
    unsigned bad = 0;
    if ((rc = cc_validate(d_i, d_j, m, nullptr, n, 0, align256(static_cast<char *>(d_work)), L, &bad, stream)) != DA_OK) return rc;
    if (bad) return fail(DA_ERR_BAD_ARG, "components: an edge endpoint is outside [0, n)");
  }
  int32_t *parent = nullptr;
  if ((rc = launch_cc_init(n, d_work, work_bytes, &parent, stream)) != DA_OK) return rc;
  if (m > 0) {
    hipLaunchKernelGGL(k_cc_union_edges, dim3(cc_grid(m)), dim3(CC_THREADS), 0, stream, d_i, d_j, d_code, min_code, m, parent);
    DA_HIP_TRY(hipGetLastError());
  }
  return launch_cc_finish(n, d_work, work_bytes, d_membership, d_sizes, n_components_out, stream);
}

int launch_components_csr(int64_t n, const int64_t *d_ptr, const int32_t *d_adj, bool symmetric, void *d_work, size_t work_bytes,
                          int32_t *d_membership, int32_t *d_sizes, int64_t *n_components_out, hipStream_t stream) {
  const CcLayout L(std::min<int64_t>(std::max<int64_t>(n, 0), CC_MAX_N));
  int rc;
  if ((rc = cc_check_work(n, d_work, work_bytes, L)) != DA_OK) return rc;
  long long ends[2] = {0, 0};
  DA_HIP_TRY(hipMemcpyAsync(&ends[0], d_ptr, 8, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipMemcpyAsync(&ends[1], d_ptr + n, 8, hipMemcpyDeviceToHost, stream));
  DA_HIP_TRY(hipStreamSynchronize(stream));
  const long long nnz = ends[1];
  if (ends[0] != 0 || nnz < 0) return fail(DA_ERR_BAD_ARG, "components: row pointers must start at 0 and not decrease");
  if (nnz > 0 && !d_adj) return fail(DA_ERR_BAD_ARG, "NULL device pointer");
  unsigned bad = 0;                                         // k_cc_validate: nothing below runs on a graph that fails it
  if ((rc = cc_validate(d_adj, nullptr, nnz, d_ptr, n, nnz, align256(static_cast<char *>(d_work)), L, &bad, stream)) != DA_OK) return rc;
  if (bad) return fail(DA_ERR_BAD_ARG, "components: the CSR is not valid (row pointers that decrease or leave [0, nnz], or a neighbour outside [0, n))");
  int32_t *parent = nullptr;
  if ((rc = launch_cc_init(n, d_work, work_bytes, &parent, stream)) != DA_OK) return rc;
  if (nnz > 0) {
    hipLaunchKernelGGL(k_cc_union_csr, dim3(cc_grid(n)), dim3(CC_THREADS), 0, stream, reinterpret_cast<const long long *>(d_ptr), d_adj, n,
                       symmetric ? 1 : 0, parent);
    DA_HIP_TRY(hipGetLastError());
  }
  return launch_cc_finish(n, d_work, work_bytes, d_membership, d_sizes, n_components_out, stream);
}

}  // namespace da
