// K_dyn -- the dynamics matcher (reference experiments/decompressor_cmd.py:26-188) after its band-pass.
//
//   k_wrms        :16-23, 90-96   windowed RMS at hop `hop`, window `sz` (truncated at the row's end), clip, log10
//   k_level       :97             b - mean(b) + mean(a)
//   k_uniform<kEdgeReflect> (uniform_filter.h)  :99-100  scipy.ndimage.uniform_filter1d(v, size), default mode "reflect"
//   k_dynfac      :109-143, 161-166   the Hann overlap-add of the source curve (do_sync is a constant False: every frame is its
//                 own value times one or two window values), 10^b / 10^aligned, clip to [0, 2], NaN -> 0
//   k_dynapply    :169, 182-185   np.interp onto the samples, mean over the channels, signal x gain
//
// Built with -ffp-contract=off: the overlap-add and the interpolation are numpy's, rounding by rounding, and the smoothing's
// compensated sums rely on every rounding step being a separate one.  Fixed summation orders, no atomics: two runs are
// bit-identical.
#include "par_common.h"
#include "uniform_filter.h"
#include <math.h>

namespace par {

// ---- k_wrms --------------------------------------------------------------------------------------------------------------
// Frame j covers samples [j hop, min(j hop + sz, n)).  With q = sz / hop and rem = sz % hop that is the hop-aligned pieces
// j .. j + q - 1 and the first rem samples of piece j + q (pieces end at n).  A workgroup takes kWrFrames consecutive frames of
// one row: it reads the samples of the pieces they touch once -- L lanes per piece, a lane two neighbouring samples (16 bytes)
// per step -- squares and sums them (lane-local ascending, then a fixed butterfly over the L lanes) into two partials per
// piece in LDS, S (the whole piece) and R (its first rem samples), and every frame then adds S[j] .. S[j + q - 1], R[j + q] in
// that order.  Pieces are staged kWrChunk at a time, so q is not bounded by LDS.  Redundant reads per workgroup: the q (+ 1)
// pieces past its last frame.
constexpr int kWrBlock = 256;
constexpr int kWrPer = 4;                           // frames per lane
constexpr int kWrFrames = kWrBlock * kWrPer;        // frames per workgroup
constexpr int kWrChunk = 2048;                      // piece partials per staged chunk (S and R: 32 KiB)

struct WrArgs {
  const double* x;
  double* out;
  int64_t pitch, n, F;
  int hop, sz, q, rem;
  int L;                // lanes per piece: a power of two, at most 64
  int vec;              // 16-byte loads are aligned
  int log10_out;
  double floor, log_floor;   // log10(floor) by the host's libm: a clipped frame is numpy's log10(floor) bit for bit
};

// samples o and o + 1 (0.0 past the piece's end) of the piece at xp; o < len
__device__ __forceinline__ void wr_load(const double* __restrict__ xp, int o, int len, int vec, double& v0, double& v1) {
  if (vec && o + 1 < len) {
    const double2 v = *reinterpret_cast<const double2*>(xp + o);
    v0 = v.x, v1 = v.y;
  } else {
    v0 = xp[o];
    v1 = o + 1 < len ? xp[o + 1] : 0.0;
  }
}

__global__ void __launch_bounds__(kWrBlock) k_wrms(WrArgs g) {
  __shared__ double S[kWrChunk];
  __shared__ double R[kWrChunk];
  const int tid = threadIdx.x;
  const double* __restrict__ xr = g.x + (int64_t)blockIdx.y * g.pitch;
  const int64_t j0 = (int64_t)blockIdx.x * kWrFrames;
  const int64_t j1 = j0 + kWrFrames < g.F ? j0 + kWrFrames : g.F;
  const int64_t p_end = j1 + g.q < g.F ? j1 + g.q : g.F;                // pieces [j0, p_end); piece p < F is never empty
  const int groups = kWrBlock / g.L, grp = tid / g.L, l = tid % g.L;
  double acc[kWrPer];
#pragma unroll
  for (int k = 0; k < kWrPer; ++k) acc[k] = 0.0;
  for (int64_t c0 = j0; c0 < p_end; c0 += kWrChunk) {
    const int64_t c1 = c0 + kWrChunk < p_end ? c0 + kWrChunk : p_end;
    const int count = (int)(c1 - c0);
    __syncthreads();                                                    // the previous chunk's partials have been read
    for (int pp0 = 0; pp0 < count; pp0 += groups) {                     // the same trip count in every lane (the butterfly)
      const int pp = pp0 + grp;
      double s = 0.0, r = 0.0;
      if (pp < count) {
        const int64_t base = (c0 + pp) * g.hop;
        const int len = g.n - base < g.hop ? (int)(g.n - base) : g.hop;
        for (int o = 2 * l; o < len; o += 2 * g.L) {
          double v0, v1;
          wr_load(xr + base, o, len, g.vec, v0, v1);
          const double a = v0 * v0, b = v1 * v1;
          s += a;
          s += b;
          if (o < g.rem) r += a;
          if (o + 1 < g.rem) r += b;
        }
      }
      for (int o = g.L >> 1; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, g.L);
        r += __shfl_xor(r, o, g.L);
      }
      if (l == 0 && pp < count) S[pp] = s, R[pp] = r;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kWrPer; ++k) {
      const int64_t j = j0 + tid + k * kWrBlock;
      if (j >= j1) continue;
      const int64_t lo = j > c0 ? j : c0;
      const int64_t hi = j + g.q < c1 ? j + g.q : c1;
      for (int64_t p = lo; p < hi; ++p) acc[k] += S[p - c0];
      if (g.rem > 0 && j + g.q >= c0 && j + g.q < c1) acc[k] += R[j + g.q - c0];
    }
  }
#pragma unroll
  for (int k = 0; k < kWrPer; ++k) {
    const int64_t j = j0 + tid + k * kWrBlock;
    if (j >= j1) continue;
    const int64_t left = g.n - j * g.hop;
    const double cnt = (double)(left < g.sz ? left : (int64_t)g.sz);
    const double rms = sqrt(acc[k] / cnt);
    double v;                                                           // np.clip(rms, floor, None): a NaN stays
    if (rms < g.floor) v = g.log10_out ? g.log_floor : g.floor;
    else v = g.log10_out ? log10(rms) : rms;
    g.out[(int64_t)blockIdx.y * g.F + j] = v;
  }
}

// ---- k_level -------------------------------------------------------------------------------------------------------------
// One workgroup per row: lane t sums elements t, t + 1024, .. of a and of b (ascending), a fixed 1024-leaf tree joins the lanes
// (the two levels), then out = (b - mean b) + mean a.  32 bytes per frame (a, b twice, out); a row of an album side is a few MB.  The ABI
// carries no scratch for partial sums of several workgroups per row.
constexpr int kLvBlock = 1024;
__global__ void __launch_bounds__(kLvBlock) k_level(const double* __restrict__ a, const double* b, int64_t F, double* out) {
  __shared__ double ra[kLvBlock];
  __shared__ double rb[kLvBlock];
  const int t = threadIdx.x;
  const double* ar = a + (int64_t)blockIdx.x * F;
  const double* br = b + (int64_t)blockIdx.x * F;
  double* orow = out + (int64_t)blockIdx.x * F;
  double sa = 0.0, sb = 0.0;
  int64_t i = t;
  for (; i + 3 * kLvBlock < F; i += 4 * kLvBlock) {                     // four loads of each row in flight, added in order
    const double a0 = ar[i], a1 = ar[i + kLvBlock], a2 = ar[i + 2 * kLvBlock], a3 = ar[i + 3 * kLvBlock];
    const double b0 = br[i], b1 = br[i + kLvBlock], b2 = br[i + 2 * kLvBlock], b3 = br[i + 3 * kLvBlock];
    sa += a0, sa += a1, sa += a2, sa += a3;
    sb += b0, sb += b1, sb += b2, sb += b3;
  }
  for (; i < F; i += kLvBlock) sa += ar[i], sb += br[i];
  ra[t] = sa, rb[t] = sb;
  __syncthreads();
  for (int s = kLvBlock / 2; s > 0; s >>= 1) {
    if (t < s) ra[t] += ra[t + s], rb[t] += rb[t + s];
    __syncthreads();
  }
  const double ma = ra[0] / (double)F, mb = rb[0] / (double)F;
  for (i = t; i + 3 * kLvBlock < F; i += 4 * kLvBlock) {
    const double b0 = br[i], b1 = br[i + kLvBlock], b2 = br[i + 2 * kLvBlock], b3 = br[i + 3 * kLvBlock];
    orow[i] = (b0 - mb) + ma, orow[i + kLvBlock] = (b1 - mb) + ma;
    orow[i + 2 * kLvBlock] = (b2 - mb) + ma, orow[i + 3 * kLvBlock] = (b3 - mb) + ma;
  }
  for (; i < F; i += kLvBlock) orow[i] = (br[i] - mb) + ma;
}

// ---- k_dynfac ------------------------------------------------------------------------------------------------------------
// The reference pads the curve by (ch, 2 ch) edge values, ch = corr_sz / 2, adds padded[x - ch : x + ch] * hann into zeros for
// x = ch, 2 ch, .. < F and cuts the padding off again.  Frame i lies in the windows x = k ch with k = i / ch + 1 (window index
// i % ch + ch, the falling half) and k + 1 (index i % ch, the rising half), as far as k <= K = (F - 1) / ch; both see a[i].
__global__ void __launch_bounds__(256) k_dynfac(const double* __restrict__ a, const double* __restrict__ b, int64_t F,
                                                const double* __restrict__ hann, int ch, double* __restrict__ aligned,
                                                double* __restrict__ fac) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= F) return;
  const int64_t e = (int64_t)blockIdx.y * F + i;
  const int64_t K = (F - 1) / ch, k1 = i / ch + 1;
  const int m = (int)(i - (k1 - 1) * ch);
  const double av = a[e];
  double al = 0.0;
  if (k1 <= K) al += av * hann[m + ch];
  if (k1 + 1 <= K) al += av * hann[m];
  if (aligned) aligned[e] = al;
  double f = pow(10.0, b[e]) / pow(10.0, al);
  f = f < 0.0 ? 0.0 : (f > 2.0 ? 2.0 : f);                              // np.clip(fac, 0, 2): a NaN stays ...
  fac[e] = f == f ? f : 0.0;                                            // ... and np.nan_to_num makes it 0
}

// ---- k_dynapply ----------------------------------------------------------------------------------------------------------
// A lane takes one sample of every channel: g_c = np.interp(i, j hop, fac[c]) (the slope form numpy uses, the key's own value
// on a key, the last value held from the last key on), g = (g_0 + g_1 + ..) / n_ch, out = float32(float64(sig) * g).
// 4 bytes in and 4 out per channel-sample; the factors come through the caches (hop lanes share two of them).
constexpr int kDaTile = 2048;
constexpr int kDaMaxCh = 8;
template <bool kVec2>
__global__ void __launch_bounds__(256) k_dynapply(const float* __restrict__ sig, int64_t sig_stride, int n_ch, int64_t n,
                                                  const double* __restrict__ fac, int64_t F, int hop, float* __restrict__ out,
                                                  int64_t out_stride) {
  const int64_t i0 = (int64_t)blockIdx.x * kDaTile;
  const int64_t jb = i0 / hop;                                          // the tile's first frame: the lanes divide 32-bit offsets
  const unsigned rb = (unsigned)(i0 - jb * hop);
  const double hop_d = (double)hop, ch_d = (double)n_ch;
#pragma unroll
  for (int k = 0; k < kDaTile / 256; ++k) {
    const int t = k * 256 + (int)threadIdx.x;
    const int64_t i = i0 + t;
    if (i < n) {
      const unsigned r = rb + (unsigned)t;
      const unsigned dj = r / (unsigned)hop, off = r - dj * (unsigned)hop;
      const int64_t j = jb + dj;
      double gsum = 0.0;
      for (int c = 0; c < n_ch; ++c) {
        const double* __restrict__ f = fac + (int64_t)c * F;
        double v;
        if (j >= F - 1) v = f[F - 1];
        else if (off == 0) v = f[j];
        else {
          const double slope = (f[j + 1] - f[j]) / hop_d;
          v = slope * (double)off + f[j];
        }
        gsum = c == 0 ? v : gsum + v;                                   // np.mean over the last axis of (n, ch): left to right
      }
      const double gain = gsum / ch_d;
      if (kVec2) {
        const float2 v = *reinterpret_cast<const float2*>(sig + 2 * i);
        *reinterpret_cast<float2*>(out + 2 * i) = make_float2((float)((double)v.x * gain), (float)((double)v.y * gain));
      } else {
        for (int c = 0; c < n_ch; ++c) out[i * out_stride + c] = (float)((double)sig[i * sig_stride + c] * gain);
      }
    }
  }
}

static int wr_lanes(int hop) {
  int L = 1;
  while (L < 64 && 4 * L <= hop) L *= 2;                                // the largest power of two <= hop / 2, within a wave
  return L;
}

}  // namespace par

extern "C" int par_windowed_rms_log10_f64(int device, const double* x, int64_t x_pitch, int64_t rows, int64_t n, int hop, int sz,
                                          double floor, int log10_out, double* out, void* stream) {
  using namespace par;
  PAR_REQUIRE(x && out, PAR_ERR_ARG, "par_windowed_rms_log10_f64: null pointer");
  PAR_REQUIRE(rows >= 1 && rows <= 65535 && n >= 1 && hop >= 1 && sz >= 1, PAR_ERR_ARG,
              "par_windowed_rms_log10_f64: bad sizes (rows %lld, n %lld, hop %d, sz %d)", (long long)rows, (long long)n, hop, sz);
  PAR_REQUIRE(x_pitch >= n, PAR_ERR_ARG, "par_windowed_rms_log10_f64: x_pitch %lld < n %lld", (long long)x_pitch, (long long)n);
  PAR_REQUIRE(!(floor != floor), PAR_ERR_ARG, "par_windowed_rms_log10_f64: floor is NaN");
  WrArgs g;
  g.x = x, g.out = out, g.pitch = x_pitch, g.n = n, g.F = ceil_div(n, hop);
  g.hop = hop, g.sz = sz, g.q = sz / hop, g.rem = sz % hop, g.L = wr_lanes(hop);
  g.vec = hop % 2 == 0 && x_pitch % 2 == 0 && ((uintptr_t)x & 15) == 0;
  g.log10_out = log10_out != 0, g.floor = floor, g.log_floor = log10(floor);
  PAR_REQUIRE(ceil_div(g.F, kWrFrames) <= 0x7fffffff, PAR_ERR_UNSUPPORTED, "par_windowed_rms_log10_f64: too many frames");
  PAR_HIP_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_wrms, dim3((unsigned)ceil_div(g.F, kWrFrames), (unsigned)rows), dim3(kWrBlock), 0, as_stream(stream), g);
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}

extern "C" int par_level_match_f64(int device, const double* a, const double* b, int64_t rows, int64_t F, double* out_b, void* stream) {
  using namespace par;
  PAR_REQUIRE(a && b && out_b, PAR_ERR_ARG, "par_level_match_f64: null pointer");
  PAR_REQUIRE(a != out_b, PAR_ERR_ARG, "par_level_match_f64: out_b is a");
  PAR_REQUIRE(rows >= 1 && rows <= 0x7fffffff && F >= 1, PAR_ERR_ARG, "par_level_match_f64: bad sizes (rows %lld, F %lld)",
              (long long)rows, (long long)F);
  PAR_HIP_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_level, dim3((unsigned)rows), dim3(kLvBlock), 0, as_stream(stream), a, b, F, out_b);
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}

extern "C" int par_uniform_filter_reflect_f64(int device, const double* in, int64_t rows, int64_t n, int size, double* out, void* stream) {
  using namespace par;
  PAR_REQUIRE(in && out, PAR_ERR_ARG, "par_uniform_filter_reflect_f64: null pointer");
  PAR_REQUIRE(in != out, PAR_ERR_ARG, "par_uniform_filter_reflect_f64: in place is not supported");
  PAR_REQUIRE(rows >= 1 && rows <= 65535 && n >= 1 && size >= 1, PAR_ERR_ARG,
              "par_uniform_filter_reflect_f64: bad sizes (rows %lld, n %lld, size %d)", (long long)rows, (long long)n, size);
  // size 1: every output is its own direct sum (the input, bit for bit); else segments as par_uniform_filter_nearest_f64
  const int64_t seg = size == 1 ? 1 : (size > 256 ? size : 256);
  const int64_t n_seg = ceil_div(n, seg);
  PAR_REQUIRE(ceil_div(n_seg, 256) <= 0x7fffffff, PAR_ERR_UNSUPPORTED, "par_uniform_filter_reflect_f64: row too long");
  PAR_HIP_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_uniform<kEdgeReflect>, dim3((unsigned)ceil_div(n_seg, 256), (unsigned)rows), dim3(256), 0, as_stream(stream), in,
                     n, size, seg, n_seg, out);
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}

extern "C" int par_dynamics_factor_f64(int device, const double* a, const double* b, int64_t rows, int64_t F, const double* hann,
                                       int corr_sz, double* aligned_or_null, double* fac, void* stream) {
  using namespace par;
  PAR_REQUIRE(a && b && hann && fac, PAR_ERR_ARG, "par_dynamics_factor_f64: null pointer");
  PAR_REQUIRE(rows >= 1 && rows <= 65535 && F >= 1, PAR_ERR_ARG, "par_dynamics_factor_f64: bad sizes (rows %lld, F %lld)",
              (long long)rows, (long long)F);
  PAR_REQUIRE(corr_sz >= 2 && corr_sz % 2 == 0, PAR_ERR_ARG, "par_dynamics_factor_f64: corr_sz %d is not an even number >= 2", corr_sz);
  PAR_REQUIRE(ceil_div(F, 256) <= 0x7fffffff, PAR_ERR_UNSUPPORTED, "par_dynamics_factor_f64: too many frames");
  PAR_HIP_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_dynfac, dim3((unsigned)ceil_div(F, 256), (unsigned)rows), dim3(256), 0, as_stream(stream), a, b, F, hann,
                     corr_sz / 2, aligned_or_null, fac);
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}

extern "C" int par_dynamics_apply_f32(int device, const float* sig, int64_t sig_stride, int n_ch, int64_t n, const double* fac,
                                      int64_t F, int hop, float* out, int64_t out_stride, void* stream) {
  using namespace par;
  PAR_REQUIRE(sig && fac && out, PAR_ERR_ARG, "par_dynamics_apply_f32: null pointer");
  PAR_REQUIRE(sig != out, PAR_ERR_ARG, "par_dynamics_apply_f32: in place is not supported");
  PAR_REQUIRE(n >= 1 && hop >= 1 && n_ch >= 1, PAR_ERR_ARG, "par_dynamics_apply_f32: bad sizes (n %lld, hop %d, channels %d)",
              (long long)n, hop, n_ch);
  PAR_REQUIRE(n_ch <= kDaMaxCh, PAR_ERR_UNSUPPORTED, "par_dynamics_apply_f32: %d channels, at most %d", n_ch, kDaMaxCh);
  PAR_REQUIRE(sig_stride >= n_ch && out_stride >= n_ch, PAR_ERR_ARG, "par_dynamics_apply_f32: stride %lld / %lld < channels %d",
              (long long)sig_stride, (long long)out_stride, n_ch);
  PAR_REQUIRE(F == ceil_div(n, hop), PAR_ERR_ARG, "par_dynamics_apply_f32: F %lld, n %lld at hop %d has %lld frames", (long long)F,
              (long long)n, hop, (long long)ceil_div(n, hop));
  PAR_REQUIRE(ceil_div(n, kDaTile) <= 0x7fffffff, PAR_ERR_UNSUPPORTED, "par_dynamics_apply_f32: signal too long");
  PAR_HIP_CHECK(hipSetDevice(device));
  const dim3 grid((unsigned)ceil_div(n, kDaTile));
  const bool vec2 = n_ch == 2 && sig_stride == 2 && out_stride == 2 && (((uintptr_t)sig | (uintptr_t)out) & 7) == 0;
  if (vec2)
    hipLaunchKernelGGL(k_dynapply<true>, grid, dim3(256), 0, as_stream(stream), sig, sig_stride, n_ch, n, fac, F, hop, out, out_stride);
  else
    hipLaunchKernelGGL(k_dynapply<false>, grid, dim3(256), 0, as_stream(stream), sig, sig_stride, n_ch, n, fac, F, hop, out, out_stride);
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}
