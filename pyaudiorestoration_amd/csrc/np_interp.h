// np.interp's inner step (numpy compiled_base.c arr_interp), restated operation by operation for the kernels that
// must equal numpy bit for bit (lag.hip, pan.hip).  Files that include this are built with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

namespace par {

__device__ __forceinline__ double interp_one(double x, const double* __restrict__ xp, const double* __restrict__ fp, int64_t m) {
  if (x > xp[m - 1]) return fp[m - 1];          // right = fp[-1]
  if (x < xp[0]) return fp[0];                  // left = fp[0]
  // largest j with xp[j] <= x  (binary_search_with_guess)
  int64_t lo = 0, hi = m - 1;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (xp[mid] <= x) lo = mid; else hi = mid;
  }
  int64_t j = (xp[hi] <= x) ? hi : lo;
  if (j == m - 1) return fp[j];
  if (xp[j] == x) return fp[j];
  const double slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]);
  double r = slope * (x - xp[j]) + fp[j];
  if (isnan(r)) {
    r = slope * (x - xp[j + 1]) + fp[j + 1];
    if (isnan(r) && fp[j] == fp[j + 1]) r = fp[j];
  }
  return r;
}

}  // namespace par
