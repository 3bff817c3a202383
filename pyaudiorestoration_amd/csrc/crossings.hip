// K_zcsmooth / K_interp -- the tail of the zero-crossing flutter analysis (experiments/zerocrossing_wow.py:17-30,
// util/wow_detection.py:342-358), added at ABI 109: the spacing of consecutive sign changes (half periods, float32 like the
// reference) smoothed with a Hann kernel on the reflect-padded sequence, turned into Hz, and np.interp onto a regular grid.
//
// K_zcsmooth.  c crossings give n = c - 1 periods d[k] = (float)(crossings[k + 1] - crossings[k]) (difference in int64, one
// rounding).  The reference pads d by span on each side (np.pad mode="reflect"), convolves with span weights (np.convolve
// mode="same") and cuts the pads off again; with h = (span - 1) / 2 that is
//     smooth[i] = sum_{j < span} (double)D(i + h - j) * w[j],     D(q) = d[fold(q)],
//     fold(q): k = q mod 2 (n - 1) (non-negative); k >= n -> 2 (n - 1) - k
// which is numpy's reflection for any pad width, pads wider than the array included.  A workgroup of kTile threads owns kTile
// outputs: it stages the kTile + span - 1 periods D(b + h - span + 1 ...) as float32 and the span weights as float64 into LDS
// (at most 4 (kTile + kMaxSpan - 1) + 8 kMaxSpan = 50172 bytes), folding only where a tile reaches past an end, and each lane
// walks the taps: consecutive lanes read consecutive periods (no bank conflict), the weight is a broadcast.
// Summation order (fixed; identical between runs): four partial sums over the taps j = 0, 1, 2, 3 (mod 4), each in ascending j,
// the tail taps j >= span - span % 4 appended to partial sums 0, 1, 2 in turn, then (s0 + s1) + (s2 + s3).  Products and sums
// are float64 with separate roundings (this file is built with -ffp-contract=off).
//
// K_interp.  out[k] = np.interp(x[k], xp, fp) through np_interp.h, one thread per abscissa; a NaN abscissa passes through as in
// numpy (arr_interp tests it before anything else).
#include "par_common.h"
#include "np_interp.h"
#include <math.h>

namespace par {

constexpr int kZcsTile = 256;         // outputs (and threads) per K_zcsmooth workgroup
constexpr int kZcsMaxSpan = 4096;     // PAR_CROSSING_SMOOTH_MAX_SPAN
constexpr int kInterpBlock = 256;

__device__ __forceinline__ float zcs_period(const long long* __restrict__ crossings, int64_t k) {
  return (float)(crossings[k + 1] - crossings[k]);
}

__global__ void __launch_bounds__(kZcsTile) k_zcsmooth(const long long* __restrict__ crossings, int64_t n,
                                                        const double* __restrict__ kernel, int span, double sr, double t0,
                                                        double* __restrict__ smooth, double* __restrict__ freq,
                                                        double* __restrict__ xp, float* __restrict__ raw) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* w = reinterpret_cast<double*>(smem);                                        // [span]
  float* p = reinterpret_cast<float*>(smem + (size_t)span * sizeof(double));           // [kZcsTile + span - 1]
  const int t = threadIdx.x;
  const int64_t b = (int64_t)blockIdx.x * kZcsTile;
  const int h = (span - 1) / 2;
  const int64_t q0 = b + h - span + 1;                      // period index of p[0], before folding
  const int need = kZcsTile + span - 1;
  for (int j = t; j < span; j += kZcsTile) w[j] = kernel[j];
  if (q0 >= 0 && q0 + need <= n) {                          // interior tile: straight through
    for (int u = t; u < need; u += kZcsTile) p[u] = zcs_period(crossings, q0 + u);
  } else {
    const int64_t per = 2 * (n - 1);                        // n >= 2
    for (int u = t; u < need; u += kZcsTile) {
      int64_t k = (q0 + u) % per;
      if (k < 0) k += per;
      if (k >= n) k = per - k;
      p[u] = zcs_period(crossings, k);
    }
  }
  __syncthreads();
  const int64_t i = b + t;
  if (i >= n) return;
  // tap j reads D(i + h - j) = p[t + span - 1 - j]
  const float* pt = p + t + span - 1;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  const int main4 = span & ~3;
  for (int j = 0; j < main4; j += 4) {
    s0 = s0 + (double)pt[-j] * w[j];
    s1 = s1 + (double)pt[-j - 1] * w[j + 1];
    s2 = s2 + (double)pt[-j - 2] * w[j + 2];
    s3 = s3 + (double)pt[-j - 3] * w[j + 3];
  }
  if (main4 < span) s0 = s0 + (double)pt[-main4] * w[main4];
  if (main4 + 1 < span) s1 = s1 + (double)pt[-main4 - 1] * w[main4 + 1];
  if (main4 + 2 < span) s2 = s2 + (double)pt[-main4 - 2] * w[main4 + 2];
  const double s = (s0 + s1) + (s2 + s3);
  if (smooth) smooth[i] = s;
  freq[i] = (sr / 2.0) / s;
  xp[i] = (double)crossings[i] / sr + t0;
  if (raw) raw[i] = (float)(sr / 2.0) / pt[-h];            // D(i) = p[t + span - 1 - h]
}

__global__ void __launch_bounds__(kInterpBlock) k_interp(const double* __restrict__ x, int64_t nx, const double* __restrict__ xp,
                                                          const double* __restrict__ fp, int64_t m, double* __restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * kInterpBlock + threadIdx.x;
  if (k >= nx) return;
  const double v = x[k];
  out[k] = (v != v && m > 1) ? v : interp_one(v, xp, fp, m);     // a one-knot table gives fp[0] to a NaN too, as numpy's does
}

}  // namespace par

extern "C" int par_crossing_smooth_f64(int device, const int64_t* crossings, int64_t c, const double* kernel, int span, double sr,
                                       double t0, double* smooth, double* freq, double* xp, float* raw, void* stream) {
  using namespace par;
  PAR_REQUIRE(crossings && kernel && freq && xp, PAR_ERR_ARG, "par_crossing_smooth_f64: null pointer");
  PAR_REQUIRE(c >= 3, PAR_ERR_ARG, "par_crossing_smooth_f64: %lld crossings, need at least 3", (long long)c);
  PAR_REQUIRE(span >= 1 && span <= kZcsMaxSpan, PAR_ERR_ARG, "par_crossing_smooth_f64: span %d outside [1, %d]", span, kZcsMaxSpan);
  PAR_REQUIRE(isfinite(sr) && sr > 0.0, PAR_ERR_ARG, "par_crossing_smooth_f64: sample rate must be finite and positive");
  const int64_t n = c - 1;
  const int64_t blocks = ceil_div(n, kZcsTile);
  PAR_REQUIRE(blocks <= 0x7fffffffLL, PAR_ERR_ARG, "par_crossing_smooth_f64: %lld crossings are too many", (long long)c);
  PAR_HIP_CHECK(hipSetDevice(device));
  const size_t lds = (size_t)span * sizeof(double) + (size_t)(kZcsTile + span - 1) * sizeof(float);
  hipLaunchKernelGGL(k_zcsmooth, dim3((unsigned)blocks), dim3(kZcsTile), lds, as_stream(stream),
                     reinterpret_cast<const long long*>(crossings), n, kernel, span, sr, t0, smooth, freq, xp, raw);
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}

extern "C" int par_interp_f64(int device, const double* x, int64_t nx, const double* xp, const double* fp, int64_t m, double* out,
                              void* stream) {
  using namespace par;
  PAR_REQUIRE(xp && fp && (nx == 0 || (x && out)), PAR_ERR_ARG, "par_interp_f64: null pointer");
  PAR_REQUIRE(m >= 1 && nx >= 0, PAR_ERR_ARG, "par_interp_f64: need m >= 1 knots and nx >= 0 (got %lld, %lld)", (long long)m,
              (long long)nx);
  if (nx == 0) return PAR_OK;
  const int64_t blocks = ceil_div(nx, kInterpBlock);
  PAR_REQUIRE(blocks <= 0x7fffffffLL, PAR_ERR_ARG, "par_interp_f64: nx %lld is too large", (long long)nx);
  PAR_HIP_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_interp, dim3((unsigned)blocks), dim3(kInterpBlock), 0, as_stream(stream), x, nx, xp, fp, m, out);
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}
