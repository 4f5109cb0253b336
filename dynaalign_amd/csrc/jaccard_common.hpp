// jaccard_common.hpp -- what the short and the long exact-Jaccard rectangle kernels share (jaccard_kernels.hip, jaccard_long_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace da {

// the tile of workgroup b when only the tiles on and above the diagonal of a T x T tile grid are launched, row by row
__device__ __forceinline__ void jc_upper_tile(unsigned b, int T, int &tr, int &tc) {
  const double w = 2.0 * T + 1.0;
  int t = (int)((w - sqrt(w * w - 8.0 * (double)b)) * 0.5);
  if (t < 0) t = 0;
  if (t > T - 1) t = T - 1;
  auto first = [T](int q) { return (long long)q * T - (long long)q * (q - 1) / 2; };   // first workgroup of tile row q
  while (t > 0 && first(t) > (long long)b) --t;
  while (t + 1 < T && first(t + 1) <= (long long)b) ++t;
  tr = t;
  tc = t + (int)((long long)b - first(t));
}

}  // namespace da
