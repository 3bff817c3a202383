// K_expand -- the Spectral Expander (reference expander_gui.py) and the time-averaged spectra of util/spectrum_flat.py.
//
//   k_mean_db_frames  spectrum_flat.py:20-24: to_dB of a magnitude block, summed over its frames per bin (the temporal mean's
//                     numerator; the caller divides by the frame count once all chunks are in)
//   k_uniform<kEdgeNearest> (uniform_filter.h) expander_gui.py:134: scipy.ndimage.uniform_filter1d(v, size, mode="nearest") along rows
//   k_expand_gain     expander_gui.py:184-197: clip -> to_fac -> np.interp onto the samples -> signal x factor
//   k_sum_rows        expander_gui.py:201: lp + hp (float64) stored into the float32 (n, ch) signal
//   k_absmax / k_div  util/units.py:32-39 normalize: d /= max|d|
// The band curve itself comes out of the STFT kernel (stft.hip, k_stft mode 2): no spectrogram is built.
//
// Built with -ffp-contract=off: the interpolation is numpy's (slope * (x - xp[j]) + fp[j], two roundings) and the smoothing's
// compensated sums rely on every rounding step being a separate one.
#include "par_common.h"
#include "db_math.h"
#include "uniform_filter.h"
#include <math.h>

namespace par {

// thread (bin lane, frame lane): 64 consecutive bins per workgroup (coalesced rows), 4 frame lanes that take every 4th frame;
// the four partials meet in LDS in lane order -- the sum does not depend on the launch
constexpr int kMeanBins = 64, kMeanLanes = 4;
// kDb: the summand is 20 log10(mag) (the temporal mean of dB); otherwise mag itself (the renoiser's selection profile, ABI 108)
template <bool kDb>
__global__ void __launch_bounds__(kMeanBins * kMeanLanes) k_mean_db_frames(const float* __restrict__ mag, int64_t n_frames, int64_t bins,
                                                                           int64_t pitch, double* __restrict__ acc) {
  __shared__ double part[kMeanLanes][kMeanBins];
  const int bl = threadIdx.x % kMeanBins, fl = threadIdx.x / kMeanBins;
  const int64_t b = (int64_t)blockIdx.x * kMeanBins + bl;
  double s = 0.0;
  if (b < bins)
    for (int64_t f = fl; f < n_frames; f += kMeanLanes) s += kDb ? 20.0 * log10_pos((double)mag[f * pitch + b]) : (double)mag[f * pitch + b];
  part[fl][bl] = s;
  __syncthreads();
  if (fl == 0 && b < bins) {
    double t = part[0][bl];
#pragma unroll
    for (int l = 1; l < kMeanLanes; ++l) t += part[l][bl];
    acc[b] += t;
  }
}

// Gain stage, kExpandTile samples of one channel per workgroup.  The factors of the frames the tile touches
// (10^((hi - clip(curve, lo, hi)) / 20), util/units.py:28-29) are computed once into LDS, then every sample takes
// np.interp(i, j * hop, fac) and the product with its sample in float64.
constexpr int kExpandTile = 1024;
__global__ void __launch_bounds__(256) k_expand_gain(const float* __restrict__ sig, int64_t sig_stride, int64_t n,
                                                     const double* __restrict__ curve, int64_t frames, int hop, double lo, double hi,
                                                     float* __restrict__ out_f32, int64_t out_stride, double* __restrict__ out_f64,
                                                     int n_ch) {
  __shared__ double fac[kExpandTile + 2];
  const int c = blockIdx.y;
  const int64_t i0 = (int64_t)blockIdx.x * kExpandTile;
  const int64_t i_last = (i0 + kExpandTile < n ? i0 + kExpandTile : n) - 1;
  // frames [j0, j1]: the tile's first frame to the right neighbour of its last sample, both clamped to the curve (a tile
  // past the curve's end only needs its last value)
  const int64_t j0 = i0 / hop < frames - 1 ? i0 / hop : frames - 1;
  const int64_t j1 = i_last / hop + 1 < frames - 1 ? i_last / hop + 1 : frames - 1;
  const double* cv = curve + (int64_t)c * frames;
  for (int64_t j = j0 + threadIdx.x; j <= j1; j += blockDim.x) {
    double d = cv[j];
    d = d < lo ? lo : (d > hi ? hi : d);                            // np.clip
    fac[j - j0] = pow(10.0, (hi - d) / 20.0);
  }
  __syncthreads();
  for (int64_t i = i0 + threadIdx.x; i <= i_last; i += blockDim.x) {
    const int64_t j = i / hop;
    double g;
    if (j >= frames - 1) {
      g = fac[frames - 1 - j0];                                     // at and past the last frame: its value (np.interp's right)
    } else if (i == j * hop) {
      g = fac[j - j0];                                              // on a frame: its value, as np.interp -- a NaN neighbour stays out
    } else {
      const double slope = (fac[j + 1 - j0] - fac[j - j0]) / (double)hop;
      g = slope * ((double)i - (double)(j * hop)) + fac[j - j0];
    }
    const double s = (double)sig[i * sig_stride + c];
    if (out_f64) {
      out_f64[(int64_t)c * n + i] = s * g;
      out_f64[((int64_t)n_ch + c) * n + i] = s;                     // the low-pass input: the channel as it was
    } else {
      out_f32[i * out_stride + c] = (float)(s * g);
    }
  }
}

__global__ void k_sum_rows(const double* __restrict__ a, const double* __restrict__ b, int64_t n, float* __restrict__ out,
                           int64_t out_stride) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t c = blockIdx.y;
  out[i * out_stride + c] = (float)(a[c * n + i] + b[c * n + i]);
}

// max |d| (NaN wins, like np.max): grid-stride partials, one per workgroup, in a fixed tree; max is order-free anyway
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || a > b) ? a : b; }
constexpr int kNormBlocks = PAR_NORMALIZE_SCRATCH_BYTES / (int)sizeof(float);
__device__ __forceinline__ float block_max(float m, float* red) {
  red[threadIdx.x] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = nan_max(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  return red[0];
}
__global__ void __launch_bounds__(256) k_absmax(const float* __restrict__ d, int64_t count, float* __restrict__ part) {
  __shared__ float red[256];
  float m = 0.0f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) m = nan_max(fabsf(d[i]), m);
  m = block_max(m, red);
  if (threadIdx.x == 0) part[blockIdx.x] = m;
}
__global__ void __launch_bounds__(256) k_div(float* __restrict__ d, int64_t count, const float* __restrict__ part, int n_part) {
  __shared__ float red[256];
  float m = 0.0f;
  for (int p = threadIdx.x; p < n_part; p += 256) m = nan_max(part[p], m);
  m = block_max(m, red);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) d[i] = d[i] / m;
}

}  // namespace par

extern "C" int par_mean_db_frames_f32(int device, const float* mag, int64_t n_frames, int64_t bins, int64_t mag_pitch, double* acc,
                                      void* stream) {
  using namespace par;
  PAR_REQUIRE(mag && acc, PAR_ERR_ARG, "par_mean_db_frames_f32: null pointer");
  PAR_REQUIRE(n_frames >= 0 && bins >= 1 && (mag_pitch == 0 || mag_pitch >= bins), PAR_ERR_ARG,
              "par_mean_db_frames_f32: bad sizes (frames %lld, bins %lld, pitch %lld)", (long long)n_frames, (long long)bins,
              (long long)mag_pitch);
  PAR_REQUIRE(ceil_div(bins, kMeanBins) <= 0x7fffffff, PAR_ERR_UNSUPPORTED, "par_mean_db_frames_f32: too many bins");
  if (n_frames == 0) return PAR_OK;
  PAR_HIP_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_mean_db_frames<true>, dim3((unsigned)ceil_div(bins, kMeanBins)), dim3(kMeanBins * kMeanLanes), 0, as_stream(stream), mag,
                     n_frames, bins, mag_pitch ? mag_pitch : bins, acc);
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}

// renoiser_gui.py:327-345 (selection profile): acc[b] += sum over f < n_frames of mag[f * mag_pitch + b], float64, the same fixed
// order as par_mean_db_frames_f32
extern "C" int par_mean_mag_frames_f32(int device, const float* mag, int64_t n_frames, int64_t bins, int64_t mag_pitch, double* acc,
                                       void* stream) {
  using namespace par;
  PAR_REQUIRE(mag && acc, PAR_ERR_ARG, "par_mean_mag_frames_f32: null pointer");
  PAR_REQUIRE(n_frames >= 0 && bins >= 1 && (mag_pitch == 0 || mag_pitch >= bins), PAR_ERR_ARG,
              "par_mean_mag_frames_f32: bad sizes (frames %lld, bins %lld, pitch %lld)", (long long)n_frames, (long long)bins,
              (long long)mag_pitch);
  PAR_REQUIRE(ceil_div(bins, kMeanBins) <= 0x7fffffff, PAR_ERR_UNSUPPORTED, "par_mean_mag_frames_f32: too many bins");
  if (n_frames == 0) return PAR_OK;
  PAR_HIP_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_mean_db_frames<false>, dim3((unsigned)ceil_div(bins, kMeanBins)), dim3(kMeanBins * kMeanLanes), 0,
                     as_stream(stream), mag, n_frames, bins, mag_pitch ? mag_pitch : bins, acc);
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}

extern "C" int par_uniform_filter_nearest_f64(int device, const double* in, int64_t rows, int64_t n, int size, double* out, void* stream) {
  using namespace par;
  PAR_REQUIRE(in && out, PAR_ERR_ARG, "par_uniform_filter_nearest_f64: null pointer");
  PAR_REQUIRE(in != out, PAR_ERR_ARG, "par_uniform_filter_nearest_f64: in place is not supported");
  PAR_REQUIRE(rows >= 1 && rows <= 65535 && n >= 1 && size >= 1 && (size % 2) == 1, PAR_ERR_ARG,
              "par_uniform_filter_nearest_f64: bad sizes (rows %lld, n %lld, size %d: odd size >= 1)", (long long)rows, (long long)n, size);
  const int64_t seg = size > 256 ? size : 256;
  const int64_t n_seg = ceil_div(n, seg);
  PAR_HIP_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_uniform<kEdgeNearest>, dim3((unsigned)ceil_div(n_seg, 256), (unsigned)rows), dim3(256), 0, as_stream(stream), in, n, size,
                     seg, n_seg, out);
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}

extern "C" int par_expand_gain_f32(int device, const float* sig, int64_t sig_stride, int n_ch, int64_t n, const double* curve,
                                   int64_t frames, int hop, double clip_lower, double clip_upper, float* out_f32, int64_t out_stride,
                                   double* out_f64, void* stream) {
  using namespace par;
  PAR_REQUIRE(sig && curve && (out_f32 || out_f64), PAR_ERR_ARG, "par_expand_gain_f32: null pointer");
  PAR_REQUIRE(n >= 1 && frames >= 1 && hop >= 1 && n_ch >= 1 && n_ch <= 65535 && sig_stride >= n_ch, PAR_ERR_ARG,
              "par_expand_gain_f32: bad sizes (n %lld, frames %lld, hop %d, channels %d, stride %lld)", (long long)n, (long long)frames, hop,
              n_ch, (long long)sig_stride);
  PAR_REQUIRE(out_f64 || out_stride >= n_ch, PAR_ERR_ARG, "par_expand_gain_f32: out_stride %lld < channels", (long long)out_stride);
  PAR_REQUIRE(ceil_div(n, kExpandTile) <= 0x7fffffff, PAR_ERR_UNSUPPORTED, "par_expand_gain_f32: signal too long");
  PAR_HIP_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_expand_gain, dim3((unsigned)ceil_div(n, kExpandTile), (unsigned)n_ch), dim3(256), 0, as_stream(stream), sig, sig_stride,
                     n, curve, frames, hop, clip_lower, clip_upper, out_f64 ? nullptr : out_f32, out_stride, out_f64, n_ch);
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}

extern "C" int par_sum_rows_f64_f32(int device, const double* a, const double* b, int n_ch, int64_t n, float* out, int64_t out_stride,
                                    void* stream) {
  using namespace par;
  PAR_REQUIRE(a && b && out, PAR_ERR_ARG, "par_sum_rows_f64_f32: null pointer");
  PAR_REQUIRE(n >= 1 && n_ch >= 1 && n_ch <= 65535 && out_stride >= n_ch, PAR_ERR_ARG, "par_sum_rows_f64_f32: bad sizes");
  PAR_HIP_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_sum_rows, dim3((unsigned)ceil_div(n, 256), (unsigned)n_ch), dim3(256), 0, as_stream(stream), a, b, n, out, out_stride);
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}

extern "C" int par_normalize_f32(int device, float* d, int64_t count, void* scratch, void* stream) {
  using namespace par;
  PAR_REQUIRE(d && scratch, PAR_ERR_ARG, "par_normalize_f32: null pointer");
  PAR_REQUIRE(count >= 1, PAR_ERR_ARG, "par_normalize_f32: empty array");
  const int blocks = (int)(ceil_div(count, 256 * 16) < kNormBlocks ? ceil_div(count, 256 * 16) : kNormBlocks);
  float* part = static_cast<float*>(scratch);
  PAR_HIP_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_absmax, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), d, count, part);
  PAR_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_div, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), d, count, part, blocks);
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}
