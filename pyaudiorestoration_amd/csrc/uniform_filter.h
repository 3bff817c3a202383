// scipy.ndimage.uniform_filter1d along rows of float64, shared by expander.hip (mode "nearest", odd sizes) and dynamics.hip
// (mode "reflect", any size).  Both include it from a file built with -ffp-contract=off: the compensated sums rely on every
// rounding step being a separate one.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace par {

// Neumaier's compensated running sum: the window sum of every output is exact to about an ulp whatever the window length
// (a plain running sum drifts with the number of slides)
struct CompSum {
  double s = 0.0, c = 0.0;
  __device__ __forceinline__ void add(double v) {
    const double t = s + v;
    c += (fabs(s) >= fabs(v)) ? (s - t) + v : (v - t) + s;
    s = t;
  }
  __device__ __forceinline__ double value() const { return s + c; }
};

constexpr int kEdgeNearest = 0;   // the edge values repeat
constexpr int kEdgeReflect = 1;   // scipy's "reflect": d c b a | a b c d | d c b a, repeated as often as the window needs

// index of the row element that position q of the extended row reads
template <int kEdge>
__device__ __forceinline__ int64_t uf_index(int64_t q, int64_t n) {
  if (q >= 0 && q < n) return q;
  if (kEdge == kEdgeNearest) return q < 0 ? 0 : n - 1;
  int64_t m = q % (2 * n);
  if (m < 0) m += 2 * n;
  return m < n ? m : 2 * n - 1 - m;
}

// One thread per segment of `seg` outputs of one row: the window sum of the segment's first output is taken directly,
// then the window slides (one sample in, one out).  seg >= size keeps the direct sum at most half of a thread's work.
// The window of output i is [i - size / 2, i + size - size / 2 - 1] (scipy's origin 0; symmetric for an odd size).
template <int kEdge>
__global__ void __launch_bounds__(256) k_uniform(const double* __restrict__ in, int64_t n, int size, int64_t seg, int64_t n_seg,
                                                 double* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_seg) return;
  const int64_t row = blockIdx.y;
  const double* x = in + row * n;
  double* y = out + row * n;
  const int64_t lo = size / 2, hi = size - size / 2 - 1;
  const int64_t i0 = t * seg, i1 = (i0 + seg < n) ? i0 + seg : n;
  auto at = [&](int64_t q) { return x[uf_index<kEdge>(q, n)]; };
  CompSum acc;
  for (int64_t q = i0 - lo; q <= i0 + hi; ++q) acc.add(at(q));
  const double inv = (double)size;
  y[i0] = acc.value() / inv;
  for (int64_t i = i0 + 1; i < i1; ++i) {
    acc.add(at(i + hi));
    acc.add(-at(i - lo - 1));
    y[i] = acc.value() / inv;
  }
}

}  // namespace par
