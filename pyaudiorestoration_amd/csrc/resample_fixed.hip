// K_rsfix -- resampling by one constant ratio: Smith's band-limited interpolation over an interpolated filter table, as
// resampy 0.4 does it (filter 'sinc_window' + interpn.resample_f with positions t * (1 / ratio)).  The four call sites of
// the reference (renoiser_gui.py:246, pytapesynch_gui.py:117-122, humspeed_gui.py:197, experiments) all use num_zeros = 8.
//
// Table (float64 on the host, held as float32):  P = 512 entries per zero crossing, N = P * Z,
//   win[j]   = hann_sym(2N + 1)[N + j] * rolloff * sinc(rolloff * j / P),  j = 0..N   (rolloff 0.945)
//   delta[j] = win[j + 1] - win[j],  delta[N] = 0
// Output t (all float64, this file is built with -ffp-contract=off so the operations round as written):
//   tr = t * inc;  n0 = int(tr);  frac = scale * (tr - n0)                      inc = 1 / ratio, scale = min(1, ratio)
//   left : idx = frac * P; off = int(idx); eta = idx - off
//          y += (win[off + i step] + eta delta[off + i step]) * x[n0 - i]       i < min(n0 + 1, (N + 1 - off) / step)
//   right: frac = scale - frac; idx, off, eta likewise
//          y += (win[off + k step] + eta delta[off + k step]) * x[n0 + k + 1]   k < min(n - n0 - 1, (N + 1 - off) / step)
// with step = int(scale * P); for ratio < 1 the sum is multiplied by scale (resampy scales its table).  n0, off and eta are
// therefore bit for bit those of the float64 statement at any position; the weights, products and sums are float32 (two
// explicit FMAs per tap).
//
// Two kernels, one output per lane, consecutive outputs per wave, grid-stride over tiles so the table is staged once per
// workgroup:
//   k_rsfix_up<8>  ratio >= 1, Z = 8: step = P, so a lane's taps are the fixed column {off, off + P, ...}.  The table sits in
//                  LDS phase-major, row `off` = (win, delta) of its Z taps, rows padded from 64 to 80 bytes so that the
//                  16-byte slots of different rows spread over all 16 slots of the bank row; a lane reads its 8 + 8 weights
//                  with eight ds_read_b128.  x comes through the vector cache: per tap a wave reads <= 65 consecutive samples.
//   k_rsfix_any    every other case: the strided walk over the natural table [j] = (win, delta), in LDS while it fits 64 KB
//                  (Z <= 15), else through the caches.
#include "par_common.h"
#include "resample_fixed.h"
#include <math.h>
#include <map>

namespace par {

constexpr int kRsUpZ = 8;
constexpr int kRsRow = 2 * kRsUpZ + 4;       // floats per phase row: 16 used + 4 of padding (80 bytes)
constexpr int kRsRows = kRsP + 1;            // off = 0..P (P itself: the right wing of an output that falls on a sample)
constexpr int kRsUpBlock = 512, kRsAnyBlock = 256;
constexpr int kRsCUs = 256;                  // gfx950

void rs_build_table(int Z, std::vector<float2>* nat, std::vector<float>* phase) {
  const int64_t N = (int64_t)kRsP * Z;
  std::vector<double> win(N + 1);
  // scipy.signal.get_window("hann", 2N + 1, fftbins=False)[N + j] = 0.5 + 0.5 cos(fac), fac = linspace(-pi, pi, 2N + 1)[N + j]
  const double fstep = (M_PI - -M_PI) / (double)(2 * N);
  for (int64_t j = 0; j <= N; ++j) {
    const double fac = j == N ? M_PI : (double)(N + j) * fstep + -M_PI;
    const double taper = 0.5 + 0.5 * cos(fac);
    const double xa = kRsRolloff * ((double)j / (double)kRsP);
    const double px = M_PI * (xa == 0.0 ? 1.0e-20 : xa);          // numpy's sinc
    win[j] = taper * (kRsRolloff * (sin(px) / px));
  }
  nat->resize(N + 1);
  for (int64_t j = 0; j <= N; ++j) (*nat)[j] = make_float2((float)win[j], j < N ? (float)(win[j + 1] - win[j]) : 0.0f);
  if (!phase) return;
  phase->assign((size_t)kRsRows * kRsRow, 0.0f);
  if (Z != kRsUpZ) return;
  for (int off = 0; off < kRsRows; ++off)
    for (int i = 0; i < Z; ++i) {
      const int64_t j = off + (int64_t)i * kRsP;
      if (j > N) continue;                                         // tap Z - 1 of row P: past the table, never used
      (*phase)[(size_t)off * kRsRow + 2 * i] = (*nat)[j].x;
      (*phase)[(size_t)off * kRsRow + 2 * i + 1] = (*nat)[j].y;
    }
}

struct RsArgs {
  const float* x;
  int64_t n, xs;
  float* y;
  int64_t n_out, ys;
  double inc, scale;
  int step, nwin;
};

// one wing with every tap bounds-checked: the signal's ends cut the wings, nothing is read outside x[0, n)
__device__ __forceinline__ float rs_wing_checked(const float2* __restrict__ tab, int off, float eta, int step, int count,
                                                 const float* __restrict__ x, int64_t n, int64_t xs, int64_t first, int dir) {
  float acc = 0.0f;
  for (int i = 0; i < count; ++i) {
    const int64_t m = first + (int64_t)dir * i;
    if (m < 0 || m >= n) continue;
    const float2 wd = tab[off + i * step];
    acc = fmaf(fmaf(eta, wd.y, wd.x), x[m * xs], acc);
  }
  return acc;
}

template <int Z>
__global__ __launch_bounds__(kRsUpBlock) void k_rsfix_up(const float4* __restrict__ phase_tab, RsArgs a) {
  extern __shared__ float4 rs_lds4[];
  for (int i = threadIdx.x; i < kRsRows * kRsRow / 4; i += kRsUpBlock) rs_lds4[i] = phase_tab[i];
  __syncthreads();
  const int64_t tiles = (a.n_out + kRsUpBlock - 1) / kRsUpBlock;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t t = tile * kRsUpBlock + threadIdx.x;
    if (t >= a.n_out) continue;
    const double tr = (double)t * a.inc;
    const int64_t n0 = (int64_t)tr;
    const double frac = tr - (double)n0;                 // scale == 1
    const double idx_l = frac * (double)kRsP;
    const int off_l = (int)idx_l;
    const float eta_l = (float)(idx_l - (double)off_l);
    const double idx_r = (1.0 - frac) * (double)kRsP;
    const int off_r = (int)idx_r;
    const float eta_r = (float)(idx_r - (double)off_r);
    // (N + 1 - off) / P taps per wing: Z for off <= 1, else Z - 1
    const int cnt_l = Z - (off_l >= 2), cnt_r = Z - (off_r >= 2);
    const float4* row_l = rs_lds4 + off_l * (kRsRow / 4);
    const float4* row_r = rs_lds4 + off_r * (kRsRow / 4);
    float acc_l = 0.0f, acc_r = 0.0f;
    if (n0 >= Z - 1 && n0 + Z < a.n) {                   // both wings whole: x[n0 - (Z - 1)] .. x[n0 + Z] exist
      const float* xl = a.x + n0 * a.xs;
      const float* xr = xl + a.xs;
#pragma unroll
      for (int q = 0; q < Z / 2; ++q) {
        const float4 wl = row_l[q], wr = row_r[q];
        const float xl0 = xl[-(int64_t)(2 * q) * a.xs], xl1 = xl[-(int64_t)(2 * q + 1) * a.xs];
        const float xr0 = xr[(int64_t)(2 * q) * a.xs], xr1 = xr[(int64_t)(2 * q + 1) * a.xs];
        acc_l = fmaf(fmaf(eta_l, wl.y, wl.x), xl0, acc_l);
        acc_r = fmaf(fmaf(eta_r, wr.y, wr.x), xr0, acc_r);
        if (2 * q + 1 < Z - 1) {
          acc_l = fmaf(fmaf(eta_l, wl.w, wl.z), xl1, acc_l);
          acc_r = fmaf(fmaf(eta_r, wr.w, wr.z), xr1, acc_r);
        } else {                                         // tap Z - 1 exists for off <= 1 only
          if (cnt_l == Z) acc_l = fmaf(fmaf(eta_l, wl.w, wl.z), xl1, acc_l);
          if (cnt_r == Z) acc_r = fmaf(fmaf(eta_r, wr.w, wr.z), xr1, acc_r);
        }
      }
    } else {
      const float* sl = reinterpret_cast<const float*>(row_l);
      const float* sr = reinterpret_cast<const float*>(row_r);
      for (int i = 0; i < cnt_l; ++i) {
        const int64_t m = n0 - i;
        if (m >= 0 && m < a.n) acc_l = fmaf(fmaf(eta_l, sl[2 * i + 1], sl[2 * i]), a.x[m * a.xs], acc_l);
      }
      for (int k = 0; k < cnt_r; ++k) {
        const int64_t m = n0 + k + 1;
        if (m >= 0 && m < a.n) acc_r = fmaf(fmaf(eta_r, sr[2 * k + 1], sr[2 * k]), a.x[m * a.xs], acc_r);
      }
    }
    a.y[t * a.ys] = acc_l + acc_r;
  }
}

template <bool LDS>
__global__ __launch_bounds__(kRsAnyBlock) void k_rsfix_any(const float2* __restrict__ nat_tab, RsArgs a) {
  extern __shared__ float2 rs_lds2[];
  const float2* tab = nat_tab;
  if (LDS) {
    for (int i = threadIdx.x; i < a.nwin; i += kRsAnyBlock) rs_lds2[i] = nat_tab[i];
    __syncthreads();
    tab = rs_lds2;
  }
  const int64_t tiles = (a.n_out + kRsAnyBlock - 1) / kRsAnyBlock;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t t = tile * kRsAnyBlock + threadIdx.x;
    if (t >= a.n_out) continue;
    const double tr = (double)t * a.inc;
    const int64_t n0 = (int64_t)tr;
    const double frac = a.scale * (tr - (double)n0);
    const double idx_l = frac * (double)kRsP;
    const int off_l = (int)idx_l;
    const float eta_l = (float)(idx_l - (double)off_l);
    const double idx_r = (a.scale - frac) * (double)kRsP;
    const int off_r = (int)idx_r;
    const float eta_r = (float)(idx_r - (double)off_r);
    const int cnt_l = (a.nwin - off_l) / a.step, cnt_r = (a.nwin - off_r) / a.step;
    float acc_l, acc_r;
    if (n0 >= cnt_l - 1 && n0 + cnt_r < a.n) {           // both wings whole
      acc_l = acc_r = 0.0f;
      const float* xl = a.x + n0 * a.xs;
      const float* xr = xl + a.xs;
      const float2* tl = tab + off_l;
      const float2* tr2 = tab + off_r;
#pragma unroll 4
      for (int i = 0; i < cnt_l; ++i) {
        const float2 wd = tl[i * a.step];
        acc_l = fmaf(fmaf(eta_l, wd.y, wd.x), xl[-(int64_t)i * a.xs], acc_l);
      }
#pragma unroll 4
      for (int k = 0; k < cnt_r; ++k) {
        const float2 wd = tr2[k * a.step];
        acc_r = fmaf(fmaf(eta_r, wd.y, wd.x), xr[(int64_t)k * a.xs], acc_r);
      }
    } else {
      acc_l = rs_wing_checked(tab, off_l, eta_l, a.step, cnt_l, a.x, a.n, a.xs, n0, -1);
      acc_r = rs_wing_checked(tab, off_r, eta_r, a.step, cnt_r, a.x, a.n, a.xs, n0 + 1, +1);
    }
    a.y[t * a.ys] = (float)((double)(acc_l + acc_r) * a.scale);
  }
}

// ---- host side: per-(device, Z) tables, kept like K_sinc's tap tables and the STFT twiddles -----------------------------
struct RsTable {
  float2* nat = nullptr;     // [N + 1] (win, delta)
  float4* phase = nullptr;   // Z = 8 only: [P + 1][kRsRow] floats
};
static std::mutex g_rs_mu;
static std::map<std::pair<int, int>, RsTable> g_rs_tabs;

static int get_rs_table(int device, int Z, RsTable* out) {
  std::lock_guard<std::mutex> lk(g_rs_mu);
  const auto key = std::make_pair(device, Z);
  auto it = g_rs_tabs.find(key);
  if (it != g_rs_tabs.end()) {
    *out = it->second;
    return PAR_OK;
  }
  std::vector<float2> nat;
  std::vector<float> phase;
  rs_build_table(Z, &nat, Z == kRsUpZ ? &phase : nullptr);
  RsTable t;
  PAR_HIP_CHECK(hipMalloc(&t.nat, nat.size() * sizeof(float2)));
  PAR_HIP_CHECK(hipMemcpy(t.nat, nat.data(), nat.size() * sizeof(float2), hipMemcpyHostToDevice));
  if (Z == kRsUpZ) {
    PAR_HIP_CHECK(hipMalloc(&t.phase, phase.size() * sizeof(float)));
    PAR_HIP_CHECK(hipMemcpy(t.phase, phase.data(), phase.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  g_rs_tabs[key] = t;
  *out = t;
  return PAR_OK;
}

}  // namespace par

extern "C" int64_t par_resample_fixed_out_len(int64_t n, double sr_orig, double sr_new) {
  if (n < 0 || !isfinite(sr_orig) || !isfinite(sr_new) || !(sr_orig > 0.0) || !(sr_new > 0.0)) return -1;
  const double v = (double)n * sr_new / sr_orig;       // int(n * sr_new / sr_orig), left to right
  if (!(v < 9.0e18)) return -1;
  return (int64_t)v;
}

extern "C" int par_resample_fixed_f32(int device, const float* x, int64_t n, int64_t x_stride, double sr_orig, double sr_new,
                                      int num_zeros, float* y, int64_t n_out, int64_t y_stride, void* stream) {
  using namespace par;
  PAR_REQUIRE(x && y, PAR_ERR_ARG, "par_resample_fixed_f32: null pointer");
  PAR_REQUIRE(isfinite(sr_orig) && isfinite(sr_new) && sr_orig > 0.0 && sr_new > 0.0, PAR_ERR_ARG,
              "par_resample_fixed_f32: sample rates must be finite and positive (got %g -> %g)", sr_orig, sr_new);
  PAR_REQUIRE(num_zeros >= 1 && num_zeros <= kRsMaxZeros, PAR_ERR_ARG, "par_resample_fixed_f32: num_zeros %d outside 1..%d",
              num_zeros, kRsMaxZeros);
  PAR_REQUIRE(x_stride >= 1 && y_stride >= 1, PAR_ERR_ARG, "par_resample_fixed_f32: strides must be >= 1");
  PAR_REQUIRE(n >= 0, PAR_ERR_ARG, "par_resample_fixed_f32: negative length");
  const int64_t want = par_resample_fixed_out_len(n, sr_orig, sr_new);
  PAR_REQUIRE(n_out == want, PAR_ERR_ARG, "par_resample_fixed_f32: n_out %lld, par_resample_fixed_out_len gives %lld",
              (long long)n_out, (long long)want);
  PAR_REQUIRE((const void*)x != (const void*)y, PAR_ERR_ARG, "par_resample_fixed_f32: x and y are the same buffer");
  if (n == 0 || n_out == 0) return PAR_OK;
  const double ratio = sr_new / sr_orig;
  PAR_REQUIRE(ratio >= 1.0 / 16.0 && ratio <= 16.0, PAR_ERR_UNSUPPORTED,
              "par_resample_fixed_f32: ratio %g outside [1/16, 16]", ratio);
  RsArgs a;
  a.x = x, a.n = n, a.xs = x_stride, a.y = y, a.n_out = n_out, a.ys = y_stride;
  a.inc = 1.0 / ratio;
  a.scale = ratio < 1.0 ? ratio : 1.0;
  a.step = (int)(a.scale * (double)kRsP);
  a.nwin = kRsP * num_zeros + 1;
  PAR_HIP_CHECK(hipSetDevice(device));
  RsTable tab;
  const int rc = get_rs_table(device, num_zeros, &tab);
  if (rc != PAR_OK) return rc;
  hipStream_t s = as_stream(stream);
  if (num_zeros == kRsUpZ && ratio >= 1.0) {
    const int64_t tiles = ceil_div(n_out, kRsUpBlock);
    const unsigned grid = (unsigned)(tiles < 3 * kRsCUs ? tiles : 3 * kRsCUs);          // three 40 KB tables per CU
    hipLaunchKernelGGL((k_rsfix_up<kRsUpZ>), dim3(grid), dim3(kRsUpBlock), kRsRows * kRsRow * sizeof(float), s, tab.phase, a);
  } else {
    const int64_t tiles = ceil_div(n_out, kRsAnyBlock);
    const unsigned grid = (unsigned)(tiles < 4 * kRsCUs ? tiles : 4 * kRsCUs);
    const size_t lds = (size_t)a.nwin * sizeof(float2);
    if (lds <= 64 * 1024)
      hipLaunchKernelGGL((k_rsfix_any<true>), dim3(grid), dim3(kRsAnyBlock), lds, s, tab.nat, a);
    else
      hipLaunchKernelGGL((k_rsfix_any<false>), dim3(grid), dim3(kRsAnyBlock), 0, s, tab.nat, a);
  }
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}
