// components_common.hpp -- the union step of the connected components, shared by components_kernels.hip (edge lists, CSR rows) and the LSH
// tail (lsh_kernels.hip k_lsh_union).  Everything here has internal linkage.
//
// parent[] is a forest over the vertices 0 .. n - 1, held in 32-bit words.  At every instant, whatever the other lanes of the launch do:
//   (I1) parent[x] <= x;
//   (I2) parent[x] is a vertex of x's component (of the graph of the edges handed to cc_union so far);
//   (I3) a vertex that has stopped being a root (parent[x] != x) never becomes one again, and its parent only ever decreases.
// The only writes are the compare-and-swap below (root hi -> a smaller root lo of the same component once the edge is counted) and the
// compression after the last union (parent[x] -> x's root, which is <= parent[x]); both keep the three.  Hence a tree's root is the
// smallest of its vertices, and once every edge has been united each component has exactly one root, its minimum: the labels do not
// depend on the order in which lanes, waves or workgroups arrive.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace da {
namespace {

// Parent words are written by every workgroup of the launch -- by the agent-scope compare-and-swap, which decides at the memory side, and by
// the agent-scope store of the compression.  The WALK reads them through the caches (a relaxed load of wavefront scope: a plain
// global_load the compiler may neither hoist nor merge): a word changes once in the union launch, from x to its parent, so a cached copy
// holds either the word's present value or x itself -- the walk then stops early at a vertex that was a root, and the swap, which expects a
// root, fails and hands back the present parent.  A stale read costs a retry, never a wrong hook.  Reading every word at agent scope
// instead sends all lanes of a large component to one memory channel for the root's word: measured 3.0 ms for 1.2·10⁶ kept pairs.
__device__ __forceinline__ int32_t cc_load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ void cc_store(int32_t *p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The read-only find: no path shortening (DESIGN.md section 7 says why).  Every step goes to a strictly smaller vertex (I1), so the walk
// ends after at most x steps; the vertex returned WAS a root when its word was read.
__device__ __forceinline__ int32_t cc_find(const int32_t *parent, int32_t x) {
  int32_t p = cc_load(parent + x);
  while (p != x) {
    x = p;
    p = cc_load(parent + x);
  }
  return x;
}

// Count the edge (a, b): afterwards a and b hang under one root.  0 <= a, b < n is the caller's business (k_cc_validate, or ids the
// library made itself).
// TERMINATION.  Lock-free: no lane ever waits for another lane to do something.  The loop leaves when the two roots are equal or when the
// compare-and-swap hooks hi under lo.  It repeats only when the swap FAILED, which means parent[hi] != hi: another lane hooked hi in
// between, the swap returned that parent `seen` < hi (I1, I3), and the next round starts from find(seen) <= seen < hi and find(lo) <= lo.
// So hi + lo strictly decreases with every failed swap and the loop runs at most a + b times for this edge; over the whole launch every
// failed swap is paid for by a parent word that strictly decreased, and those decreases are bounded by the sum of the vertex numbers.
__device__ __forceinline__ void cc_union(int32_t *parent, int32_t a, int32_t b) {
  a = cc_find(parent, a);
  b = cc_find(parent, b);
  while (a != b) {
    const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const int32_t seen = atomicCAS(parent + hi, hi, lo);   // expects hi to be a root still; lo < hi keeps (I1)
    if (seen == hi) return;
    a = cc_find(parent, seen);
    b = cc_find(parent, lo);
  }
}

}  // namespace
}  // namespace da
