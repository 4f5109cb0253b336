// components.cpp -- da_components: connected components of an edge list on the host (clusterbreak.components_dense, element for element).
// The CPU twin of components_kernels.hip: the fallback for small graphs and what runs without a device.  A union-find whose hooks go
// larger root -> smaller root, so a tree's root is the smallest of its vertices; the walk of find halves its path with grandparents, which
// are smaller still.  Ids from 1 in order of first appearance are then the roots numbered in vertex order.
#include <cstdint>
#include <vector>

#include "da_common.hpp"

namespace da {
namespace {

inline int32_t uf_find(std::vector<int32_t> &parent, int32_t x) {
  while (parent[(size_t)x] != x) {
    const int32_t g = parent[(size_t)parent[(size_t)x]];
    parent[(size_t)x] = g;
    x = g;
  }
  return x;
}

}  // namespace
}  // namespace da

using namespace da;

extern "C" int da_components(int64_t n, int64_t n_edges, const int32_t *ei, const int32_t *ej, int32_t *membership_out, int64_t *n_components_out) {
  if (n < 0 || n_edges < 0 || n > 0x7ffffff0LL) return fail(DA_ERR_BAD_ARG, "bad vertex / edge count");
  if (!n_components_out) return fail(DA_ERR_BAD_ARG, "NULL pointer");
  if (n > 0 && !membership_out) return fail(DA_ERR_BAD_ARG, "NULL membership buffer");
  if (n_edges > 0 && (!ei || !ej)) return fail(DA_ERR_BAD_ARG, "NULL edge arrays");
  *n_components_out = 0;
  if (n == 0) return DA_OK;
  for (int64_t e = 0; e < n_edges; ++e)                     // before anything indexes by an endpoint
    if (ei[e] < 0 || ei[e] >= n || ej[e] < 0 || ej[e] >= n)
      return fail(DA_ERR_BAD_ARG, "components: edge %lld (%d, %d) has an endpoint outside [0, %lld)", (long long)e, (int)ei[e], (int)ej[e], (long long)n);
  std::vector<int32_t> parent((size_t)n);
  for (int64_t v = 0; v < n; ++v) parent[(size_t)v] = (int32_t)v;
  for (int64_t e = 0; e < n_edges; ++e) {
    const int32_t a = uf_find(parent, ei[e]), b = uf_find(parent, ej[e]);
    if (a != b) parent[(size_t)(a > b ? a : b)] = a > b ? b : a;
  }
  int32_t next_id = 0;                                      // parent[v] < v is a vertex of v's component and has its id already
  for (int64_t v = 0; v < n; ++v) {
    const int32_t p = parent[(size_t)v];
    membership_out[v] = p == v ? ++next_id : membership_out[p];
  }
  *n_components_out = next_id;
  return DA_OK;
}
