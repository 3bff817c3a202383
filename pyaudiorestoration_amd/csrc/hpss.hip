// K_hpss -- median-filtering harmonic / percussive separation (reference util/decompose.py hpss / harmonic / softmask, driven by
// experiments/hpss_gui.py), ABI 109.
//
//   k_hpss      per bin of a frame-major spectrogram: harm = median of |S| over win_harm frames, perc = median of |S| over
//               win_perc bins (scipy.ndimage.median_filter, mode "reflect"), the two soft masks and S x mask
//   k_residual  r = x - (h + p) per sample (hpss_gui.py:145)
//
// One workgroup owns a tile of 64 frames x 64 bins.  It stages the magnitudes of the tile plus win_perc - 1 halo bins in LDS
// (transposed: a row per bin, a column per frame), selects the frequency-direction medians with lanes on frames, leaves them in
// a 64 x 64 LDS array, then stages the tile plus win_harm - 1 halo frames into the same LDS region (a row per frame, a column per
// bin) and selects the time-direction medians with lanes on bins.  Rows are 65 floats apart, so the transposed stores, the
// column reads of the selection and the transposed read of the finished medians are all free of bank conflicts.
//
// Selection: a median is the element of rank k/2, and non-negative floats order like their bit patterns, so the answer is built
// from bit 30 down: bit b stays set when fewer than rank + 1 window elements lie below the candidate.  31 passes over the window
// whatever k is (1..99), no per-k code and no register array of k elements.  A lane selects kRun consecutive outputs of its column
// at once: their windows overlap in all but kRun - 1 elements, so one LDS read feeds kRun compare-and-count pairs.
//
// Built with -ffp-contract=off: the mask's a*a + b*b and S x mask round every step separately, as numpy does (the one fused
// product of numpy's complex64 x float32 is spelled as an fmaf: np_mul_c64_f32).
#include "par_common.h"
#include "np_abs.h"
#include <math.h>
#include <cmath>

namespace par {

constexpr int kHpssTile = 64;                 // frames and bins per tile (= lanes of a wave)
constexpr int kHpssRow = kHpssTile + 1;       // LDS row stride in floats
constexpr int kHpssThreads = 256;
constexpr int kHpssWaves = kHpssThreads / kWave;
constexpr int kHpssRun = 4;                   // consecutive outputs a lane selects together
constexpr int kHpssMaxWin = 99;

enum { kPowGeneral = 0, kPowOne = 1, kPowTwo = 2, kPowHalf = 3, kPowHard = 4 };
enum { kOutComponents = 0, kOutMasks = 1, kOutHarmonic = 2, kOutMedians = 3 };

struct HpssParams {
  int64_t n_frames, bins, pitch;
  int win_harm, win_perc;
  int pow_mode, out_kind;
  float power, margin_h, margin_p, bad_value;
};

// scipy's "reflect" (half-sample symmetric, d c b a | a b c d | d c b a), repeated as often as the halo needs.  Only positions
// off the axis pay for the 64-bit remainder: those are the halos of the tiles at an edge.
__device__ __forceinline__ int64_t reflect_index(int64_t p, int64_t n) {
  if (p >= 0 && p < n) return p;
  const int64_t period = 2 * n;
  int64_t m = p % period;
  if (m < 0) m += period;
  return m < n ? m : period - 1 - m;
}

template <bool kComplex>
__device__ __forceinline__ float load_mag(const void* __restrict__ spec, int64_t idx) {
  if (kComplex) {
    const float2 v = static_cast<const float2*>(spec)[idx];
    return np_abs_c64(v.x, v.y);
  }
  return fabsf(static_cast<const float*>(spec)[idx]);                // magnitudes: the sign bit must be clear for the bit-pattern order
}

// Rank-`rank` elements of the kHpssRun windows col[(i + j) * kHpssRow], j < k, i < kHpssRun (bit patterns of non-negative floats)
__device__ __forceinline__ void select_run(const uint32_t* __restrict__ col, int k, int rank, uint32_t (&ans)[kHpssRun]) {
#pragma unroll
  for (int i = 0; i < kHpssRun; ++i) ans[i] = 0u;
  const int span = k + kHpssRun - 1;
  const int head = kHpssRun - 1 < span ? kHpssRun - 1 : span;       // j < head: not yet inside every window
  const int tail = k > kHpssRun - 1 ? k : kHpssRun - 1;             // j >= tail: already past some window
  for (uint32_t bit = 0x40000000u; bit; bit >>= 1) {
    uint32_t t[kHpssRun];
    int cnt[kHpssRun];
#pragma unroll
    for (int i = 0; i < kHpssRun; ++i) {
      t[i] = ans[i] | bit;
      cnt[i] = 0;
    }
    for (int j = 0; j < head; ++j) {
      const uint32_t v = col[j * kHpssRow];
#pragma unroll
      for (int i = 0; i < kHpssRun; ++i)
        if (j >= i && j - i < k) cnt[i] += v < t[i];
    }
#pragma unroll 4
    for (int j = head; j < tail; ++j) {                             // inside all kHpssRun windows (empty when k < kHpssRun)
      const uint32_t v = col[j * kHpssRow];
#pragma unroll
      for (int i = 0; i < kHpssRun; ++i) cnt[i] += v < t[i];
    }
    for (int j = tail; j < span; ++j) {
      const uint32_t v = col[j * kHpssRow];
#pragma unroll
      for (int i = 0; i < kHpssRun; ++i)
        if (j >= i && j - i < k) cnt[i] += v < t[i];
    }
#pragma unroll
    for (int i = 0; i < kHpssRun; ++i)
      if (cnt[i] <= rank) ans[i] = t[i];                            // at most `rank` elements below t: the answer is >= t
  }
}

// decompose.softmask in float32: Z = max(X, Xref); Z < FLT_MIN (subnormals included, whatever the denormal mode: the bit
// patterns are compared) -> bad_value; else (X/Z)^p / ((X/Z)^p + (Xref/Z)^p); the hard mask is X > Xref (false on a NaN).
// np.maximum keeps a NaN where fmaxf drops it: a NaN in X or Xref makes Z, both ratios and the mask NaN, also beside an
// Xref or X under FLT_MIN, where fmaxf alone would answer bad_value.
__device__ __forceinline__ float softmask(float x, float xref, int pow_mode, float power, float bad_value) {
  if (pow_mode == kPowHard) return x > xref ? 1.0f : 0.0f;
  if (x != x || xref != xref) return __builtin_nanf("");
  const float z = fmaxf(x, xref);
  if (__float_as_uint(z) < 0x00800000u) return bad_value;
  float a = x / z, b = xref / z;
  if (pow_mode == kPowTwo) {                                        // numpy's float32 ** 2.0 squares
    a = a * a;
    b = b * b;
  } else if (pow_mode == kPowHalf) {                                // ... and ** 0.5 takes the square root
    a = sqrtf(a);
    b = sqrtf(b);
  } else if (pow_mode == kPowGeneral) {
    a = powf(a, power);
    b = powf(b, power);
  }
  return a / (a + b);
}

// numpy's complex64 * float32: the mask is promoted to m + 0i and the full complex product is formed, in numpy's vector loop as
// re = fma(s.re, m, -(s.im * 0)), im = fma(s.re, 0, s.im * m) = s.re * 0 + s.im * m.  For finite non-zero parts that is
// (s.re * m, s.im * m); the products with the 0 make both parts NaN when either part of S is infinite or NaN and decide the sign
// of a zero result, and the one fused product keeps the sign of a real part that underflows.
__device__ __forceinline__ float2 np_mul_c64_f32(float2 s, float m) {
  return make_float2(fmaf(s.x, m, -(s.y * 0.0f)), s.x * 0.0f + s.y * m);
}

template <bool kComplex>
__global__ __launch_bounds__(kHpssThreads) void k_hpss(const void* __restrict__ spec, HpssParams p, void* __restrict__ out_h,
                                                       void* __restrict__ out_p) {
  extern __shared__ float lds[];
  const int kmax = p.win_harm > p.win_perc ? p.win_harm : p.win_perc;
  float* tile = lds;                                                // [kHpssTile + kmax - 1][kHpssRow]
  float* perc_t = lds + (kHpssTile + kmax - 1) * kHpssRow;          // [bin][frame], kHpssRow apart
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int64_t f0 = (int64_t)blockIdx.x * kHpssTile, b0 = (int64_t)blockIdx.y * kHpssTile;
  const int nf = (int)(p.n_frames - f0 < kHpssTile ? p.n_frames - f0 : kHpssTile);     // frames and bins of this tile
  const int nb = (int)(p.bins - b0 < kHpssTile ? p.bins - b0 : kHpssTile);

  // ---- frequency direction: tile[r][f] = |S[f0 + f][reflect(b0 - win_perc/2 + r)]|, lanes along r (coalesced rows)
  {
    const int rows = kHpssTile + p.win_perc - 1;
    const int64_t first = b0 - p.win_perc / 2;
    for (int f = wave; f < kHpssTile; f += kHpssWaves) {
      const int64_t frame = f < nf ? f0 + f : p.n_frames - 1;       // columns past the last frame are never written out
      for (int r = lane; r < rows; r += kWave)
        tile[r * kHpssRow + f] = load_mag<kComplex>(spec, frame * p.pitch + reflect_index(first + r, p.bins));
    }
    __syncthreads();
    const uint32_t* col = reinterpret_cast<const uint32_t*>(tile) + lane;
    for (int o = wave * kHpssRun; o < nb; o += kHpssWaves * kHpssRun) {
      uint32_t m[kHpssRun];
      select_run(col + o * kHpssRow, p.win_perc, p.win_perc / 2, m);
#pragma unroll
      for (int i = 0; i < kHpssRun; ++i) perc_t[(o + i) * kHpssRow + lane] = __uint_as_float(m[i]);
    }
    __syncthreads();
  }

  // ---- time direction: tile[r][b] = |S[reflect(f0 - win_harm/2 + r)][b0 + b]|, lanes along b
  const int rows = kHpssTile + p.win_harm - 1;
  const int64_t first = f0 - p.win_harm / 2;
  const int64_t bin = lane < nb ? b0 + lane : p.bins - 1;
  for (int r = wave; r < rows; r += kHpssWaves) tile[r * kHpssRow + lane] = load_mag<kComplex>(spec, reflect_index(first + r, p.n_frames) * p.pitch + bin);
  __syncthreads();
  const uint32_t* col = reinterpret_cast<const uint32_t*>(tile) + lane;
  for (int o = wave * kHpssRun; o < nf; o += kHpssWaves * kHpssRun) {
    uint32_t m[kHpssRun];
    select_run(col + o * kHpssRow, p.win_harm, p.win_harm / 2, m);
    if (lane >= nb) continue;
#pragma unroll
    for (int i = 0; i < kHpssRun; ++i) {
      if (o + i >= nf) break;
      const float harm = __uint_as_float(m[i]);
      const float perc = perc_t[lane * kHpssRow + o + i];
      const int64_t idx = (f0 + o + i) * p.pitch + b0 + lane;
      if (p.out_kind == kOutMedians) {
        static_cast<float*>(out_h)[idx] = harm;
        static_cast<float*>(out_p)[idx] = perc;
        continue;
      }
      const float mh = softmask(harm, perc * p.margin_h, p.pow_mode, p.power, p.bad_value);
      const float mp = p.out_kind == kOutHarmonic ? 0.0f : softmask(perc, harm * p.margin_p, p.pow_mode, p.power, p.bad_value);
      if (p.out_kind == kOutMasks) {
        static_cast<float*>(out_h)[idx] = mh;
        static_cast<float*>(out_p)[idx] = mp;
      } else if (kComplex) {
        const float2 s = static_cast<const float2*>(spec)[idx];
        static_cast<float2*>(out_h)[idx] = np_mul_c64_f32(s, mh);
        if (p.out_kind == kOutComponents) static_cast<float2*>(out_p)[idx] = np_mul_c64_f32(s, mp);
      } else {
        const float s = static_cast<const float*>(spec)[idx];
        static_cast<float*>(out_h)[idx] = s * mh;
        if (p.out_kind == kOutComponents) static_cast<float*>(out_p)[idx] = s * mp;
      }
    }
  }
}

__global__ void k_residual(const float* __restrict__ x, int64_t x_stride, const float* __restrict__ h, int64_t h_stride,
                           const float* __restrict__ p, int64_t p_stride, int64_t n, float* __restrict__ r, int64_t r_stride) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  r[i * r_stride] = x[i * x_stride] - (h[i * h_stride] + p[i * p_stride]);
}

}  // namespace par

extern "C" int par_hpss_f32(int device, const void* spec, int is_complex, int64_t n_frames, int64_t bins, int64_t pitch, int win_harm,
                            int win_perc, double power, double margin_h, double margin_p, void* out_h, void* out_p, int out_kind,
                            void* stream) {
  using namespace par;
  PAR_REQUIRE(out_kind >= kOutComponents && out_kind <= kOutMedians, PAR_ERR_ARG, "par_hpss_f32: out_kind %d outside 0..3", out_kind);
  PAR_REQUIRE(spec && out_h && (out_p || out_kind == kOutHarmonic), PAR_ERR_ARG, "par_hpss_f32: null pointer");
  PAR_REQUIRE(out_h != spec && out_p != spec && out_h != out_p, PAR_ERR_ARG, "par_hpss_f32: in place is not supported (every bin reads its neighbours)");
  PAR_REQUIRE(win_harm >= 1 && win_harm <= kHpssMaxWin && win_perc >= 1 && win_perc <= kHpssMaxWin, PAR_ERR_ARG,
              "par_hpss_f32: kernel sizes (%d, %d) outside 1..%d", win_harm, win_perc, kHpssMaxWin);
  PAR_REQUIRE(power > 0.0, PAR_ERR_ARG, "par_hpss_f32: power must be strictly positive (got %g)", power);
  PAR_REQUIRE(margin_h >= 1.0 && margin_p >= 1.0, PAR_ERR_ARG, "par_hpss_f32: margins must be >= 1.0 (got %g, %g)", margin_h, margin_p);
  const int64_t pt = pitch ? pitch : bins;
  PAR_REQUIRE(n_frames >= 0 && bins >= 1 && pt >= bins, PAR_ERR_ARG, "par_hpss_f32: bad sizes (frames %lld, bins %lld, pitch %lld)",
              (long long)n_frames, (long long)bins, (long long)pitch);
  PAR_REQUIRE(ceil_div(n_frames, kHpssTile) <= 0x7fffffff && ceil_div(bins, kHpssTile) <= 65535, PAR_ERR_UNSUPPORTED,
              "par_hpss_f32: spectrogram too large");
  if (n_frames == 0) return PAR_OK;
  HpssParams p;
  p.n_frames = n_frames;
  p.bins = bins;
  p.pitch = pt;
  p.win_harm = win_harm;
  p.win_perc = win_perc;
  p.out_kind = out_kind;
  p.power = (float)power;
  p.pow_mode = std::isinf(power) ? kPowHard : power == 1.0 ? kPowOne : power == 2.0 ? kPowTwo : power == 0.5 ? kPowHalf : kPowGeneral;
  p.margin_h = (float)margin_h;
  p.margin_p = (float)margin_p;
  p.bad_value = (margin_h == 1.0 && margin_p == 1.0) ? 0.5f : 0.0f;
  const int kmax = win_harm > win_perc ? win_harm : win_perc;
  const size_t lds = (size_t)((kHpssTile + kmax - 1) * kHpssRow + kHpssTile * kHpssRow) * sizeof(float);     // at most 58760 bytes
  const dim3 grid((unsigned)ceil_div(n_frames, kHpssTile), (unsigned)ceil_div(bins, kHpssTile));
  PAR_HIP_CHECK(hipSetDevice(device));
  if (is_complex)
    hipLaunchKernelGGL(k_hpss<true>, grid, dim3(kHpssThreads), lds, as_stream(stream), spec, p, out_h, out_p);
  else
    hipLaunchKernelGGL(k_hpss<false>, grid, dim3(kHpssThreads), lds, as_stream(stream), spec, p, out_h, out_p);
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}

extern "C" int par_residual_f32(int device, const float* x, int64_t x_stride, const float* h, int64_t h_stride, const float* p,
                                int64_t p_stride, int64_t n, float* r, int64_t r_stride, void* stream) {
  using namespace par;
  PAR_REQUIRE(x && h && p && r, PAR_ERR_ARG, "par_residual_f32: null pointer");
  PAR_REQUIRE(n >= 0 && x_stride >= 1 && h_stride >= 1 && p_stride >= 1 && r_stride >= 1, PAR_ERR_ARG,
              "par_residual_f32: bad sizes (n %lld, strides %lld %lld %lld %lld)", (long long)n, (long long)x_stride, (long long)h_stride,
              (long long)p_stride, (long long)r_stride);
  PAR_REQUIRE(ceil_div(n, 256) <= 0x7fffffff, PAR_ERR_UNSUPPORTED, "par_residual_f32: signal too long");
  if (n == 0) return PAR_OK;
  PAR_HIP_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_residual, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, as_stream(stream), x, x_stride, h, h_stride, p, p_stride, n, r,
                     r_stride);
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}
