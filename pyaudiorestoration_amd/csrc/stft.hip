// K_stft / K_istft -- overlapped-window real STFT (+ fused magnitude) and least-squares ISTFT.
//
// Semantics (reference util/fourier.py): stft :37-75 with the numpy/pyfftw framing --
// estimate_and_center :78-82 (reflect pad n_fft/2, n_frames = (len_pad-n_fft)//hop+1),
// segment_array :160-166 (frame = window * slice, zero-extended at the END to n_fft*zeropad),
// rfft, / sqrt(n_fft) (:157); to_mag :23-24 (|X| + 1e-7) fused as mode 1.
// istft :314-437 with window_sumsquare :492-546 and __overlap_add :677-687.
//
// CDNA4 mapping: no frame matrix is ever materialised.  A workgroup owns a few consecutive frames,
// H/8 lanes each (one wave per frame at n_fft = 1024): a lane gathers 8 complex points straight from
// the (possibly channel-strided) signal with the reflect boundary folded into the index, multiplies
// by the window (the real frame is packed as an M/2-point complex sequence), runs a Stockham autosort
// FFT with radix-8 butterflies in registers (one LDS exchange per radix-8 stage, no bit reversal),
// untangles the half-size spectrum into the M/2+1 real-FFT bins and writes them FRAME-MAJOR (bins
// contiguous -> coalesced stores).  HBM traffic is the
// algorithmic minimum: each input sample is fetched from HBM once (neighbouring frames hit L2) and
// each output bin is written once; magnitude never round-trips a complex spectrogram.
#include "par_common.h"
#include "db_math.h"
#include "np_abs.h"
#include "pan_items.h"
#include "image_tables.h"
#include "track_band.h"
#include <math.h>
#include <map>
#include <set>
#include <type_traits>
#include <vector>

namespace par {

struct Twiddles {
  float2* w = nullptr;    // exp(-2*pi*i*t/H), t = 0..H-1          (complex FFT of size H = M/2)
  float2* post = nullptr; // exp(-2*pi*i*k/M), k = 0..H            (real-FFT untangling)
};
static std::mutex g_tw_mu;

// Dynamic LDS above the 64 KB a kernel gets by default is raised per (kernel, device) once: the attribute belongs to the
// function object of the CURRENT device.
static int raise_dynamic_lds(const void* fn, int bytes, int device) {
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> done;
  if (bytes <= 65536) return PAR_OK;
  std::lock_guard<std::mutex> lk(mu);
  if (done.count({fn, device})) return PAR_OK;
  PAR_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  done.insert({fn, device});
  return PAR_OK;
}
// launch with `lds` bytes of dynamic LDS, the kernel's limit raised first where the launch needs it
template <typename... P, typename... A>
static int launch_with_lds(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, int device, hipStream_t s, A... args) {
  const int rc = raise_dynamic_lds(reinterpret_cast<const void*>(kernel), (int)lds, device);
  if (rc != PAR_OK) return rc;
  hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}
static std::map<std::pair<int, int>, Twiddles> g_tw;

static int get_twiddles(int device, int M, Twiddles* out) {
  std::lock_guard<std::mutex> lk(g_tw_mu);
  auto key = std::make_pair(device, M);
  auto it = g_tw.find(key);
  if (it != g_tw.end()) {
    *out = it->second;
    return PAR_OK;
  }
  const int H = M / 2;
  std::vector<float2> w(H), post(H + 1);
  for (int t = 0; t < H; ++t) {
    const double a = -2.0 * M_PI * (double)t / (double)H;
    w[t] = make_float2((float)cos(a), (float)sin(a));
  }
  for (int k = 0; k <= H; ++k) {
    const double a = -2.0 * M_PI * (double)k / (double)M;
    post[k] = make_float2((float)cos(a), (float)sin(a));
  }
  Twiddles t;
  PAR_HIP_CHECK(hipMalloc(&t.w, H * sizeof(float2)));
  PAR_HIP_CHECK(hipMalloc(&t.post, (H + 1) * sizeof(float2)));
  PAR_HIP_CHECK(hipMemcpy(t.w, w.data(), H * sizeof(float2), hipMemcpyHostToDevice));
  PAR_HIP_CHECK(hipMemcpy(t.post, post.data(), (H + 1) * sizeof(float2), hipMemcpyHostToDevice));
  g_tw[key] = t;
  *out = t;
  return PAR_OK;
}

__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
  return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cconj(float2 a) { return make_float2(a.x, -a.y); }
// multiply by -i (forward) : (x,y) -> (y,-x)
__device__ __forceinline__ float2 mul_mi(float2 a) { return make_float2(a.y, -a.x); }

// np.pad(x, pad, mode="reflect") index: position q relative to x[0], any q (multiple reflections).
__device__ __forceinline__ long long reflect_index(long long q, long long n) {
  if (n == 1) return 0;
  const long long P = 2 * (n - 1);
  q %= P;
  if (q < 0) q += P;
  return q < n ? q : P - q;
}

// ---- FFT core ------------------------------------------------------------------------------------------
// H-point complex Stockham autosort FFT with 8 points per lane held in REGISTERS: T = H/8 lanes per frame
// (H = 512 -> exactly one wave per frame).  Every stage consumes x[j + q*T], q = 0..7 (conflict-free
// LDS reads, and for the first stage coalesced global reads), does radix-8 butterflies in registers and
// scatters to the autosort positions; a final radix-2/4 stage covers log2(H) not divisible by 3.  LDS is
// touched log8(H) times instead of log2..log4(H) times, and indices are padded e -> e + e/8 so the
// scattered 64-bit writes are bank-conflict free.
__device__ __forceinline__ int lpad(int e) { return e + (e >> 3); }

__device__ __forceinline__ void radix2(float2& a, float2& b) {
  const float2 t = a;
  a = cadd(t, b);
  b = csub(t, b);
}
// forward 4-point DFT in place: (v0,v1,v2,v3) -> (X0,X1,X2,X3)
__device__ __forceinline__ void radix4(float2& v0, float2& v1, float2& v2, float2& v3) {
  const float2 a0 = cadd(v0, v2), a1 = csub(v0, v2), a2 = cadd(v1, v3), a3 = mul_mi(csub(v1, v3));
  v0 = cadd(a0, a2);
  v1 = cadd(a1, a3);
  v2 = csub(a0, a2);
  v3 = csub(a1, a3);
}
// forward 8-point DFT in place, natural order in and out
__device__ __forceinline__ void radix8(float2 (&v)[8]) {
  // split into even (0,2,4,6) and odd (1,3,5,7) 4-point DFTs
  float2 e0 = v[0], e1 = v[2], e2 = v[4], e3 = v[6];
  float2 o0 = v[1], o1 = v[3], o2 = v[5], o3 = v[7];
  radix4(e0, e1, e2, e3);
  radix4(o0, o1, o2, o3);
  const float h = 0.70710678118654752f;
  // odd outputs times W8^k: W8^1 = (1-i)/sqrt2, W8^2 = -i, W8^3 = (-1-i)/sqrt2
  o1 = make_float2((o1.x + o1.y) * h, (o1.y - o1.x) * h);
  o2 = mul_mi(o2);
  o3 = make_float2((o3.y - o3.x) * h, -(o3.x + o3.y) * h);
  v[0] = cadd(e0, o0);
  v[4] = csub(e0, o0);
  v[1] = cadd(e1, o1);
  v[5] = csub(e1, o1);
  v[2] = cadd(e2, o2);
  v[6] = csub(e2, o2);
  v[3] = cadd(e3, o3);
  v[7] = csub(e3, o3);
}

// The lanes of one frame exchange data through LDS.  Up to 64 lanes per frame they all sit in ONE wave, whose
// LDS operations execute in order: a compiler-level fence is enough and the waves of a workgroup never wait
// for each other; larger frames need the workgroup barrier.
template <int T>
__device__ __forceinline__ void frame_sync() {
  if constexpr (T <= kWave) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  } else {
    __syncthreads();
  }
}

// v[q] = x[j + q*T] on entry (natural order); on exit X (padded LDS frame) holds the transform in natural order.
// All lanes of the frame (for T > 64: of the workgroup) must call this together.
template <int LOGH>
__device__ __forceinline__ void fft_core(float2 (&v)[8], float2* __restrict__ X, int j, const float2* __restrict__ tw) {
  constexpr int H = 1 << LOGH, T = H / 8;
  constexpr int N8 = LOGH / 3, REM = LOGH % 3;
  // the gathered twiddle of every later stage depends only on the lane: fetch them all up front so their
  // latency hides under the first butterflies instead of sitting between the LDS exchanges
  float2 w1s[N8 > 1 ? N8 : 1];
#pragma unroll
  for (int st = 1; st < N8; ++st) {
    const int Nst = 1 << (3 * st);
    w1s[st] = tw[(j & (Nst - 1)) * (H / (Nst * 8))];
  }
  int Ns = 1;
#pragma unroll
  for (int st = 0; st < N8; ++st) {
    if (st > 0) {
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = X[lpad(j + q * T)];
    }
    const int k = j & (Ns - 1);
    if (st > 0) {
      // one gathered twiddle load per stage; the other six are its powers (3 multiply levels, ~2 ulp)
      const float2 w1 = w1s[st];
      const float2 w2 = cmul(w1, w1), w3 = cmul(w2, w1), w4 = cmul(w2, w2);
      const float2 w5 = cmul(w4, w1), w6 = cmul(w3, w3), w7 = cmul(w4, w3);
      v[1] = cmul(v[1], w1);
      v[2] = cmul(v[2], w2);
      v[3] = cmul(v[3], w3);
      v[4] = cmul(v[4], w4);
      v[5] = cmul(v[5], w5);
      v[6] = cmul(v[6], w6);
      v[7] = cmul(v[7], w7);
    }
    radix8(v);
    frame_sync<T>();                       // everybody has finished reading X
    const int base = ((j - k) << 3) + k;
#pragma unroll
    for (int r = 0; r < 8; ++r) X[lpad(base + r * Ns)] = v[r];
    frame_sync<T>();
    Ns <<= 3;
  }
  if (REM) {
    constexpr int Rl = 1 << REM, U = 8 / Rl;
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = X[lpad(j + q * T)];
    const int step = H / (Ns * Rl);
    int bk[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int b = j + u * T;
      const int k = b & (Ns - 1);
      bk[u] = ((b - k) * Rl) + k;
#pragma unroll
      for (int r = 1; r < Rl; ++r) v[u + r * U] = cmul(v[u + r * U], tw[r * k * step]);
      if (Rl == 2) radix2(v[u], v[u + U]);
      else radix4(v[u], v[u + U], v[u + 2 * U], v[u + 3 * U]);
    }
    frame_sync<T>();
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int r = 0; r < Rl; ++r) X[lpad(bk[u] + r * Ns)] = v[u + r * U];
    frame_sync<T>();
  }
}

// Workgroups are dispatched round-robin over the 8 XCDs, each with its own L2.  Overlapping frames share most of
// their input, so consecutive frame groups should meet in ONE L2: logical group g = (b % 8) * ceil(n/8) + b / 8
// gives every XCD a contiguous range of frames (groups past the end exit).
constexpr int kXcds = 8;
__device__ __forceinline__ int64_t xcd_contiguous_block(int64_t n_blocks) {
  const int64_t per = (n_blocks + kXcds - 1) / kXcds;
  return (int64_t)(blockIdx.x % kXcds) * per + blockIdx.x / kXcds;
}

template <int LOGH>
struct FftGeom {
  static constexpr int H = 1 << LOGH;
  static constexpr int T = H / 8;                               // lanes per frame
  static constexpr int Threads = T > 256 ? T : 256;
  static constexpr int Frames = Threads / T;                    // frames per workgroup
  static constexpr int FrameLds = H + H / 8 + 8;                // padded float2 slots per frame
  static constexpr int P = (H / 2) / T;                         // bin pairs (k, H - k) a lane untangles: k = j + i T, i < P
  static constexpr size_t FramesLds = (size_t)Frames * FrameLds * sizeof(float2);    // bytes of LDS of a workgroup's frames
  // workgroups for `items` frame slots: a multiple of the XCD count (xcd_contiguous_block)
  static unsigned grid(int64_t items) { return (unsigned)(ceil_div(ceil_div(items, Frames), kXcds) * kXcds); }
};

// The kernels take the transform size as log2 of H = M / 2: f(std::integral_constant<int, LOGH>{}) for LOGH = logh in [LO, HI],
// the sizes the caller's kernels exist for
template <int LO, int HI, typename F>
static int dispatch_logh(int logh, F&& f) {
  if constexpr (LO > HI) {
    PAR_REQUIRE(false, PAR_ERR_UNSUPPORTED, "stft: no kernel for transforms of 2^%d points", logh + 1);
  } else {
    return logh == LO ? f(std::integral_constant<int, LO>{}) : dispatch_logh<LO + 1, HI>(logh, f);
  }
}
// ... and a run-time flag as a bool template argument: f(std::true_type{}) or f(std::false_type{})
template <typename F>
static int dispatch_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}
static int ilog2(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

// MODE 0: complex spectrum, 1: magnitude |X| + 1e-7, 2: band dB -- out[f] (float64, `out` reinterpreted) = mean over
// b in [bin_l, bin_u) of 20 log10(the float32 magnitude mode 1 writes), with the band packed into `pitch` as
// bin_l | bin_u << 32 (the kernel's parameter list, and so the code of modes 0 and 1, stays as it was).  Mode 2 writes
// one float64 per frame: no spectrogram reaches HBM, and only the band's bins take a log.  UNIT: the signal is contiguous (x_stride == 1): no 64-bit stride
// multiply per sample and the two samples of a packed point arrive in one 8-byte load.
template <int LOGH, int MODE, bool UNIT>
__global__ __launch_bounds__(FftGeom<LOGH>::Threads) void k_stft(const float* __restrict__ x, int64_t n, int64_t x_stride_arg,
                                                                  int n_fft, int hop, const float* __restrict__ window,
                                                                  const float2* __restrict__ tw,
                                                                  const float2* __restrict__ post, float* __restrict__ out,
                                                                  int64_t n_frames, float scale, int64_t pitch) {
  const int64_t x_stride = UNIT ? 1 : x_stride_arg;
  constexpr int mode = MODE;
  using G = FftGeom<LOGH>;
  constexpr int H = G::H, T = G::T;
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  const int f = threadIdx.x / T, j = threadIdx.x - f * T;
  float2* X = lds + f * G::FrameLds;
  const int64_t fr = xcd_contiguous_block((n_frames + G::Frames - 1) / G::Frames) * G::Frames + f;
  const bool live = fr < n_frames;
  // gather + window + pack: z[i] = (xw[2i], xw[2i+1]); lanes read consecutive float pairs (coalesced)
  float2 v[8];
  const long long base = (long long)fr * hop - (n_fft >> 1);
  // interior frames (the vast majority) index the signal directly; only frames that overhang an end of
  // the signal pay for the reflect fold (a 64-bit modulo per sample)
  const bool interior = live && base >= 0 && base + n_fft <= (long long)n;
  if (interior && n_fft == 2 * H) {
    // no zero padding (the usual case): every packed pair lies inside the frame, no compare per pair
    const float* xs = x + base * x_stride;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int t0 = 2 * (j + q * T);
      const float2 w = *reinterpret_cast<const float2*>(window + t0);
      v[q] = make_float2(w.x * xs[(int64_t)t0 * x_stride], w.y * xs[(int64_t)(t0 + 1) * x_stride]);
    }
  } else if (interior) {
    const float* xs = x + base * x_stride;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int t0 = 2 * (j + q * T);
      float2 z = make_float2(0.0f, 0.0f);
      if (t0 + 1 < n_fft) {
        const float2 w = *reinterpret_cast<const float2*>(window + t0);
        z.x = w.x * xs[(int64_t)t0 * x_stride];
        z.y = w.y * xs[(int64_t)(t0 + 1) * x_stride];
      } else if (t0 < n_fft) {
        z.x = window[t0] * xs[(int64_t)t0 * x_stride];
      }
      v[q] = z;
    }
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int t0 = 2 * (j + q * T);
      float2 z = make_float2(0.0f, 0.0f);
      if (live) {
        if (t0 < n_fft) z.x = window[t0] * x[reflect_index(base + t0, n) * x_stride];
        if (t0 + 1 < n_fft) z.y = window[t0 + 1] * x[reflect_index(base + t0 + 1, n) * x_stride];
      }
      v[q] = z;
    }
  }
  // untangling twiddles W^k of this lane's bins: fetched before the FFT so they are in registers when the last
  // exchange completes.  Bins come in pairs (k, H-k) that share everything but two signs, so a lane owns
  // k = j, j+T, .. below H/2 and writes both members (lane 0 adds the self-paired bin H/2).
  constexpr int bins = H + 1, P = (H / 2) / T;
  float2 pw[P + 1];
#pragma unroll
  for (int i = 0; i < P; ++i) pw[i] = post[j + i * T];
  pw[P] = post[H / 2];
  fft_core<LOGH>(v, X, j, tw);
  if (mode != 2 && !live) return;         // mode 2 keeps every lane to the frame reduction (a workgroup barrier for T > 64)
  const float hs = 0.5f * scale;
  const int band_l = (int)(pitch & 0xffffffffll), band_u = (int)(pitch >> 32);    // mode 2 only
  double band_acc = 0.0;
  // (re, im) arrive UNSCALED (twice the bin, before the 1/sqrt(n_fft)): the complex form scales both parts, the magnitude
  // form scales once behind the square root (|hs z| = hs |z|: two multiplies per bin saved)
  auto emit = [&](int k, float re, float im) {
    // The magnitude spectrogram is consumed sparsely (tracker bands): streaming stores (get_mag 0.39 -> 0.365 ms).
    // The complex one is re-read right away by the inpaint / ISTFT kernels: regular stores (streaming ones cost
    // 2 % on the config-4 chain).
    if constexpr (mode == 0) {
      reinterpret_cast<float2*>(out)[fr * pitch + k] = make_float2(re * hs, im * hs);
    } else if constexpr (mode == 2) {
      if (k >= band_l && k < band_u)
        band_acc += 20.0 * log10_pos((double)fmaf(__builtin_amdgcn_sqrtf(fmaf(re, re, im * im)), hs, 1e-7f));
    } else {
      // v_sqrt_f32 itself (1 ulp): the correctly rounded sqrtf costs 16 instructions per bin, mostly compares and selects
      const float mag = fmaf(__builtin_amdgcn_sqrtf(fmaf(re, re, im * im)), hs, 1e-7f);
      // streaming stores pay when a frame's lanes write runs of at least 64 bytes (T >= 16: n_fft >= 256); shorter runs only
      // complete their lines together with the neighbouring frames', in L2, and went to HBM piecemeal as streaming stores
      // (n_fft = 64, hop 16 on 57.6 M samples: 0.81 ms streaming, 0.39 ms plain; n_fft = 256: 0.26 against 0.31)
      if (T < 16) out[fr * pitch + k] = mag;
      else __builtin_nontemporal_store(mag, out + fr * pitch + k);
    }
  };
  // LDS slots of the pair (k, H - k), k = j + i T: with T a multiple of 8 the padding is linear in i, so both are one
  // base per lane plus an immediate (the wrap H - 0 -> 0 only exists for lane 0's first pair)
  constexpr bool kLinearPad = (T % 8) == 0;
  constexpr int kPadStep = T + T / 8;
  const int lp_k0 = lpad(j), lp_m0 = lpad(H - j);
#pragma unroll
  for (int i = 0; i <= P; ++i) {
    const int k = (i < P) ? j + i * T : H / 2;
    if (i == P && j != 0) break;
    int sk = lpad(k), sm = lpad((H - k) & (H - 1));
    if (kLinearPad && i < P) {
      sk = lp_k0 + i * kPadStep;
      sm = (i == 0 && j == 0) ? 0 : lp_m0 - i * kPadStep;
    }
    const float2 zk = X[sk];
    const float2 zc = cconj(X[sm]);
    const float2 ev = cadd(zk, zc);                     // Z[k] + conj(Z[H-k])
    const float2 t = cmul(pw[i], csub(zk, zc));         // W^k * (Z[k] - conj(Z[H-k]))
    emit(k, ev.x + t.y, ev.y - t.x);                    // X[k]   = (ev - i*t)/2 * scale
    if (i < P) emit(H - k, ev.x - t.y, -ev.y - t.x);    // X[H-k] = (conj(ev) - i*conj(t))/2 * scale
  }
  if constexpr (mode == 2) {
    // the frame's T lanes sum in a fixed order: xor butterflies inside the wave, then (T > 64) the waves' partials in
    // wave order from LDS beside the frames
    constexpr int kLanes = T < kWave ? T : kWave;
#pragma unroll
    for (int o = kLanes / 2; o > 0; o >>= 1) band_acc += __shfl_xor(band_acc, o, kWave);
    if constexpr (T > kWave) {
      double* part = reinterpret_cast<double*>(lds + G::Frames * G::FrameLds) + f * (T / kWave);
      if ((j & (kWave - 1)) == 0) part[j / kWave] = band_acc;
      __syncthreads();
      if (j == 0) {
        band_acc = part[0];
        for (int w = 1; w < T / kWave; ++w) band_acc += part[w];
      }
    }
    if (live && j == 0) reinterpret_cast<double*>(out)[fr] = band_acc / (double)(band_u - band_l);
  }
}

// ---- stereo balance boxes straight from the two channels (pypan_gui.py:79-103) ------------------------------------------
// One frame slot of FftGeom per work item (box, frame) of pan_items.h.  The slot's lanes gather the frame of BOTH channels
// in one pass over the samples (PAIR: an interleaved stereo file, xR == xL + 1 and x_stride == 2, delivers L and R of a
// sample in one 8-byte load), transform L, keep the float32 magnitudes of the bins they own in registers, transform R
// through the same LDS frame and divide bin by bin: both magnitudes of a cell meet in the lane that owns the bin, so the
// quotient needs no exchange.  Each lane sums its quotients inside the band in float64 and counts them; the slot reduces as
// k_stft mode 2 does (xor butterflies, then the waves' partials in wave order) and writes ONE PanPart.  No spectrogram
// reaches HBM, and frames outside every box are never transformed.  Gather, window product, transform, untangle and the
// magnitude are k_stft mode 1's expressions, operation by operation.
template <int LOGH, bool PAIR>
__global__ __launch_bounds__(FftGeom<LOGH>::Threads) void k_stft_pan(const float* __restrict__ xL, const float* __restrict__ xR,
                                                                      int64_t n, int64_t x_stride, int n_fft, int hop,
                                                                      const float* __restrict__ window,
                                                                      const float2* __restrict__ tw, const float2* __restrict__ post,
                                                                      const int* __restrict__ boxes, int64_t n_box,
                                                                      const int64_t* __restrict__ offs, PanPart* __restrict__ part,
                                                                      int64_t n_items, float scale) {
  using G = FftGeom<LOGH>;
  constexpr int H = G::H, T = G::T;
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  const int f = threadIdx.x / T, j = threadIdx.x - f * T;
  float2* X = lds + f * G::FrameLds;
  const int64_t item = xcd_contiguous_block((n_items + G::Frames - 1) / G::Frames) * G::Frames + f;
  const bool live = item < n_items;            // a dead slot runs along with zeros (the transforms synchronise the workgroup)
  int band_l = 0, band_u = 0;
  long long fr = 0;
  if (live) {
    const int64_t box = pan_item_box(offs, n_box, item);
    const int* bx = boxes + 4 * box;
    band_l = bx[0];
    band_u = bx[1];
    fr = (long long)bx[2] + (item - offs[box]);
  }
  // one (L, R) pair per sample index
  auto sample = [&](long long idx) {
    if constexpr (PAIR) return *reinterpret_cast<const float2*>(xL + 2 * idx);
    else return make_float2(xL[idx * x_stride], xR[idx * x_stride]);
  };
  float2 vL[8], vR[8];
  const long long base = fr * hop - (n_fft >> 1);
  const bool interior = live && base >= 0 && base + n_fft <= (long long)n;
  if (interior && n_fft == 2 * H) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int t0 = 2 * (j + q * T);
      const float2 w = *reinterpret_cast<const float2*>(window + t0);
      const float2 s0 = sample(base + t0), s1 = sample(base + t0 + 1);
      vL[q] = make_float2(w.x * s0.x, w.y * s1.x);
      vR[q] = make_float2(w.x * s0.y, w.y * s1.y);
    }
  } else if (interior) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int t0 = 2 * (j + q * T);
      float2 zl = make_float2(0.0f, 0.0f), zr = zl;
      if (t0 + 1 < n_fft) {
        const float2 w = *reinterpret_cast<const float2*>(window + t0);
        const float2 s0 = sample(base + t0), s1 = sample(base + t0 + 1);
        zl = make_float2(w.x * s0.x, w.y * s1.x);
        zr = make_float2(w.x * s0.y, w.y * s1.y);
      } else if (t0 < n_fft) {
        const float w = window[t0];
        const float2 s0 = sample(base + t0);
        zl.x = w * s0.x;
        zr.x = w * s0.y;
      }
      vL[q] = zl;
      vR[q] = zr;
    }
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int t0 = 2 * (j + q * T);
      float2 zl = make_float2(0.0f, 0.0f), zr = zl;
      if (live) {
        if (t0 < n_fft) {
          const float w = window[t0];
          const float2 s0 = sample(reflect_index(base + t0, n));
          zl.x = w * s0.x;
          zr.x = w * s0.y;
        }
        if (t0 + 1 < n_fft) {
          const float w = window[t0 + 1];
          const float2 s1 = sample(reflect_index(base + t0 + 1, n));
          zl.y = w * s1.x;
          zr.y = w * s1.y;
        }
      }
      vL[q] = zl;
      vR[q] = zr;
    }
  }
  constexpr int P = (H / 2) / T;
  float2 pw[P + 1];
#pragma unroll
  for (int i = 0; i < P; ++i) pw[i] = post[j + i * T];
  pw[P] = post[H / 2];
  const float hs = 0.5f * scale;
  constexpr bool kLinearPad = (T % 8) == 0;
  constexpr int kPadStep = T + T / 8;
  const int lp_k0 = lpad(j), lp_m0 = lpad(H - j);
  // k_stft's untangle of the pair (k, H - k), k = j + i T (lane 0 adds the self-paired bin H/2): emit(slot, k, re, im) with the
  // lane's bins numbered slot = 2 i and 2 i + 1
  auto untangle = [&](auto&& emit) {
#pragma unroll
    for (int i = 0; i <= P; ++i) {
      const int k = (i < P) ? j + i * T : H / 2;
      if (i == P && j != 0) break;
      int sk = lpad(k), sm = lpad((H - k) & (H - 1));
      if (kLinearPad && i < P) {
        sk = lp_k0 + i * kPadStep;
        sm = (i == 0 && j == 0) ? 0 : lp_m0 - i * kPadStep;
      }
      const float2 zk = X[sk];
      const float2 zc = cconj(X[sm]);
      const float2 ev = cadd(zk, zc);
      const float2 t = cmul(pw[i], csub(zk, zc));
      emit(2 * i, k, ev.x + t.y, ev.y - t.x);
      if (i < P) emit(2 * i + 1, H - k, ev.x - t.y, -ev.y - t.x);
    }
  };
  float magl[2 * P + 1] = {};
  fft_core<LOGH>(vL, X, j, tw);
  untangle([&](int slot, int, float re, float im) { magl[slot] = fmaf(__builtin_amdgcn_sqrtf(fmaf(re, re, im * im)), hs, 1e-7f); });
  // fft_core synchronises the frame's lanes before its first store to X: the reads above are done by then
  fft_core<LOGH>(vR, X, j, tw);
  double acc = 0.0;
  int cnt = 0;
  untangle([&](int slot, int k, float re, float im) {
    if (k >= band_l && k < band_u) {
      const float magr = fmaf(__builtin_amdgcn_sqrtf(fmaf(re, re, im * im)), hs, 1e-7f);
      const float q = __fdiv_rn(magl[slot], magr);          // numpy's float32 division, correctly rounded
      if (q == q) {                                          // nanmean skips NaN cells; +-inf is summed
        acc += (double)q;
        ++cnt;
      }
    }
  });
  constexpr int kLanes = T < kWave ? T : kWave;
#pragma unroll
  for (int o = kLanes / 2; o > 0; o >>= 1) {
    acc += __shfl_xor(acc, o, kWave);
    cnt += __shfl_xor(cnt, o, kWave);
  }
  if constexpr (T > kWave) {
    double* psum = reinterpret_cast<double*>(lds + G::Frames * G::FrameLds) + f * (T / kWave);
    int* pcnt = reinterpret_cast<int*>(reinterpret_cast<double*>(lds + G::Frames * G::FrameLds) + G::Threads / kWave) + f * (T / kWave);
    if ((j & (kWave - 1)) == 0) {
      psum[j / kWave] = acc;
      pcnt[j / kWave] = cnt;
    }
    __syncthreads();
    if (j == 0) {
      acc = psum[0];
      cnt = pcnt[0];
      for (int w = 1; w < T / kWave; ++w) {
        acc += psum[w];
        cnt += pcnt[w];
      }
    }
  }
  if (live && j == 0) {
    part[item].sum = acc;
    part[item].cnt = cnt;
  }
}

// ---- time-averaged dB spectra straight from the samples (util/spectrum_flat.py:20-24 under difeq_gui.get_eq) ------------------
// A frame slot of FftGeom takes a RUN of consecutive frames of one channel: it transforms them one after the other through the
// same LDS frame and every lane adds 20 log10 of the float32 magnitudes of the bins the untangle step leaves it -- the pairs
// (k, H - k), k = j + i T, and lane 0 the self-paired bin H/2: at most 9 -- into float64 registers, frames ascending.  After the
// run the slot writes ONE partial row; k_mean_db_reduce adds the rows in run order and divides by the frame count.  No
// spectrogram reaches HBM, no atomics, and the run length depends on the frame count alone (mean_run_len), so the order of
// every sum is fixed by the arguments.  Gather, window product, transform, untangle and the magnitude are k_stft mode 1's
// expressions, operation by operation.  Every slot of the grid makes `run` passes through fft_core (workgroup barriers for
// T > 64): a pass beyond the slot's last frame transforms zeros and adds nothing.
constexpr int kMeanMinRun = 16;        // frames per run for short files: 16 transforms amortise the partial row
constexpr int kMeanMaxRuns = 512;      // longer files: at most this many partial rows per channel (twice the CUs)
static inline int64_t mean_run_len(int64_t n_frames) {
  const int64_t r = (n_frames + kMeanMaxRuns - 1) / kMeanMaxRuns;
  return r < kMeanMinRun ? kMeanMinRun : r;
}

template <int LOGH, bool UNIT>
__global__ __launch_bounds__(FftGeom<LOGH>::Threads) void k_stft_mean(const float* __restrict__ x_all, int64_t n, int64_t x_stride_arg,
                                                                       int n_fft, int hop, const float* __restrict__ window,
                                                                       const float2* __restrict__ tw, const float2* __restrict__ post,
                                                                       double* __restrict__ part, int64_t n_frames, int64_t run,
                                                                       int64_t n_runs, float scale) {
  const int64_t x_stride = UNIT ? 1 : x_stride_arg;
  using G = FftGeom<LOGH>;
  constexpr int H = G::H, T = G::T;
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  const int f = threadIdx.x / T, j0 = threadIdx.x - f * T;
  float2* X = lds + f * G::FrameLds;
  const int c = blockIdx.y;
  const float* x = x_all + c;
  const int64_t slot = xcd_contiguous_block((n_runs + G::Frames - 1) / G::Frames) * G::Frames + f;
  const bool owns = slot < n_runs;             // a slot past the last run goes along with zeros (the transforms synchronise the workgroup)
  const int64_t f_first = slot * run;
  const int64_t f_end = !owns ? f_first : (f_first + run < n_frames ? f_first + run : n_frames);
  constexpr int bins = H + 1, P = (H / 2) / T;
  float2 pw[P + 1];
#pragma unroll
  for (int i = 0; i < P; ++i) pw[i] = post[j0 + i * T];
  pw[P] = post[H / 2];
  const float hs = 0.5f * scale;
  constexpr bool kLinearPad = (T % 8) == 0;
  constexpr int kPadStep = T + T / 8;
  double acc[2 * P + 1] = {};
  for (int64_t r = 0; r < run; ++r) {
    const int64_t fr = f_first + r;
    const bool live = fr < f_end;
    float2 v[8];
    // A lane of the 1024-lane workgroup has 128 registers.  Everything a pass derives from the lane index alone -- window values,
    // stage twiddles and their powers, LDS and sample offsets -- would be kept across the loop and spill; an opaque copy of the
    // index keeps it inside the pass (integer arithmetic and L1 / L2 hits, beside nine float64 logarithms per lane).
    int j = j0;
    if constexpr (G::Threads > 512) asm volatile("" : "+v"(j));
    const int lp_k0 = lpad(j), lp_m0 = lpad(H - j);
    const long long base = (long long)fr * hop - (n_fft >> 1);
    const bool interior = live && base >= 0 && base + n_fft <= (long long)n;
    if (interior && n_fft == 2 * H) {
      const float* xs = x + base * x_stride;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int t0 = 2 * (j + q * T);
        const float2 w = *reinterpret_cast<const float2*>(window + t0);
        v[q] = make_float2(w.x * xs[(int64_t)t0 * x_stride], w.y * xs[(int64_t)(t0 + 1) * x_stride]);
      }
    } else if (interior) {
      const float* xs = x + base * x_stride;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int t0 = 2 * (j + q * T);
        float2 z = make_float2(0.0f, 0.0f);
        if (t0 + 1 < n_fft) {
          const float2 w = *reinterpret_cast<const float2*>(window + t0);
          z.x = w.x * xs[(int64_t)t0 * x_stride];
          z.y = w.y * xs[(int64_t)(t0 + 1) * x_stride];
        } else if (t0 < n_fft) {
          z.x = window[t0] * xs[(int64_t)t0 * x_stride];
        }
        v[q] = z;
      }
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int t0 = 2 * (j + q * T);
        float2 z = make_float2(0.0f, 0.0f);
        if (live) {
          if (t0 < n_fft) z.x = window[t0] * x[reflect_index(base + t0, n) * x_stride];
          if (t0 + 1 < n_fft) z.y = window[t0 + 1] * x[reflect_index(base + t0 + 1, n) * x_stride];
        }
        v[q] = z;
      }
    }
    // fft_core synchronises the frame's lanes before its first store to X: the previous frame's untangle reads are done by then
    fft_core<LOGH>(v, X, j, tw);
    if (live) {
      // the float32 magnitudes first (the LDS reads and the untangle), then the float64 logarithms
      float mg[2 * P + 1];
      auto add = [&](int s, float re, float im) { mg[s] = fmaf(__builtin_amdgcn_sqrtf(fmaf(re, re, im * im)), hs, 1e-7f); };
#pragma unroll
      for (int i = 0; i <= P; ++i) {
        const int k = (i < P) ? j + i * T : H / 2;
        if (i == P && j != 0) break;
        int sk = lpad(k), sm = lpad((H - k) & (H - 1));
        if (kLinearPad && i < P) {
          sk = lp_k0 + i * kPadStep;
          sm = (i == 0 && j == 0) ? 0 : lp_m0 - i * kPadStep;
        }
        const float2 zk = X[sk];
        const float2 zc = cconj(X[sm]);
        const float2 ev = cadd(zk, zc);
        const float2 t = cmul(pw[i], csub(zk, zc));
        add(2 * i, ev.x + t.y, ev.y - t.x);                     // bin k
        if (i < P) add(2 * i + 1, ev.x - t.y, -ev.y - t.x);     // bin H - k
      }
#pragma unroll
      for (int s = 0; s <= 2 * P; ++s) {
        if (s == 2 * P && j != 0) break;
        acc[s] += 20.0 * log10_pos((double)mg[s]);
      }
    }
  }
  if (!owns) return;
  double* row = part + ((int64_t)c * n_runs + slot) * bins;
#pragma unroll
  for (int i = 0; i < P; ++i) {
    row[j0 + i * T] = acc[2 * i];
    row[H - (j0 + i * T)] = acc[2 * i + 1];
  }
  if (j0 == 0) row[H / 2] = acc[2 * P];
}

// mean[c][b] = (part[c][0][b] + part[c][1][b] + ... in run order) / n_frames
__global__ __launch_bounds__(256) void k_mean_db_reduce(const double* __restrict__ part, int64_t n_runs, int bins, int64_t n_frames,
                                                        double* __restrict__ mean) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= bins) return;
  const int c = blockIdx.y;
  const double* p = part + (int64_t)c * n_runs * bins + b;
  double s = p[0];
#pragma unroll 8
  for (int64_t r = 1; r < n_runs; ++r) s += p[r * bins];
  mean[(int64_t)c * bins + b] = s / (double)n_frames;
}

// ---- spectrogram image straight from the samples (util/spectrum.py: the whole-file STFT reduced to a screen's pixels) ------------
// The structure of k_stft_mean with a maximum in place of the sum.  A unit is one chunk of the frames of one DISTINCT column (a
// column equal to its predecessor is served by the predecessor's units); k_image_plan turns the column table into the units'
// prefix offsets, one int64 per column, and a frame slot finds its unit's column by bisection.  The slot transforms the chunk's
// frames one after the other through one LDS frame and keeps the maxima of its at most 9 bins as unsigned integers
// (image_key: positive floats order as their bit patterns, a NaN above them all).  After the run the maxima go into the frame's
// LDS slot indexed by bin, lane j reduces rows j, j + T, ... over their bin ranges and writes them into every column of the
// group: plain stores for a column of one chunk, otherwise a vector atomic maximum on the bit patterns into the image, which
// k_image_zero has filled with 0.0f -- a maximum has no order, so the image does not depend on which chunk arrives first.
// Gather, window product, transform, untangle and the magnitude are k_stft mode 1's expressions, operation by operation.
// Slots that share a workgroup (T < 256) all make `passes` passes through fft_core, the longest chunk's frame count; a pass
// beyond a slot's last frame transforms zeros and adds nothing.  One slot per workgroup (T >= 256) makes its own chunk's passes.
__global__ __launch_bounds__(1024) void k_image_plan(const int64_t* __restrict__ cols, int64_t width, int64_t chunk, int64_t n_frames,
                                                     int64_t* __restrict__ unit_off) {
  __shared__ int64_t part[1024];
  const int t = threadIdx.x;
  const int64_t per = (width + 1023) / 1024;
  const int64_t c0 = t * per < width ? t * per : width, c1 = c0 + per < width ? c0 + per : width;
  auto chunks = [&](int64_t c) -> int64_t {
    const int64_t lo = cols[2 * c], hi = cols[2 * c + 1];
    if (lo < 0 || hi > n_frames || hi <= lo) return 0;                                   // (the host copy has been validated; the device one is not trusted)
    if (c > 0 && cols[2 * c - 2] == lo && cols[2 * c - 1] == hi) return 0;
    return (hi - lo + chunk - 1) / chunk;
  };
  int64_t own = 0;
  for (int64_t c = c0; c < c1; ++c) own += chunks(c);
  part[t] = own;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int64_t add = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  int64_t run = part[t] - own;
  for (int64_t c = c0; c < c1; ++c) {
    unit_off[c] = run;
    run += chunks(c);
  }
  if (t == 1023) unit_off[width] = part[1023];
}

__global__ __launch_bounds__(256) void k_image_zero(float* __restrict__ peak, int64_t width, int height, int64_t pitch) {
  const int r = blockIdx.y * 256 + threadIdx.x;
  if (r < height) peak[(int64_t)blockIdx.x * pitch + r] = 0.0f;
}

template <int LOGH, bool UNIT>
__global__ __launch_bounds__(FftGeom<LOGH>::Threads) void k_stft_peak_image(const float* __restrict__ x, int64_t n, int64_t x_stride_arg,
                                                                             int n_fft, int hop, const float* __restrict__ window,
                                                                             const float2* __restrict__ tw, const float2* __restrict__ post,
                                                                             const int64_t* __restrict__ cols, const int32_t* __restrict__ rows,
                                                                             const int64_t* __restrict__ unit_off, int64_t width, int height,
                                                                             float* __restrict__ peak, int64_t pitch, int64_t n_frames,
                                                                             int64_t chunk, int64_t passes_all, int64_t n_units, float scale) {
  const int64_t x_stride = UNIT ? 1 : x_stride_arg;
  using G = FftGeom<LOGH>;
  constexpr int H = G::H, T = G::T;
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  const int f = threadIdx.x / T, j0 = threadIdx.x - f * T;
  float2* X = lds + f * G::FrameLds;
  const int64_t slot = xcd_contiguous_block((n_units + G::Frames - 1) / G::Frames) * G::Frames + f;
  // the unit's column: the last c with unit_off[c] <= slot (columns without units share their successor's offset)
  bool owns = slot < n_units;
  int64_t col = 0, f_first = 0, f_end = 0, n_chunks = 0, c_lo = 0, c_hi = 0;
  if (owns) {
    int64_t lo = 0, hi = width;
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (unit_off[mid] <= slot) lo = mid; else hi = mid;
    }
    col = lo;
    c_lo = cols[2 * col];
    c_hi = cols[2 * col + 1];
    const int64_t k = slot - unit_off[col], len = c_hi - c_lo;
    owns = c_lo >= 0 && c_hi <= n_frames && len > 0;
    if (owns) {
      n_chunks = (len + chunk - 1) / chunk;
      owns = k >= 0 && k < n_chunks;
    }
    if (owns) {
      // the column's frames in n_chunks nearly equal parts
      f_first = c_lo + k * len / n_chunks;
      f_end = c_lo + (k + 1) * len / n_chunks;
    }
  }
  if (G::Frames == 1 && !owns) return;         // the workgroup's only slot: nobody waits for it
  const int64_t passes = G::Frames == 1 ? f_end - f_first : passes_all;
  constexpr int bins = H + 1, P = (H / 2) / T;
  float2 pw[P + 1];
#pragma unroll
  for (int i = 0; i < P; ++i) pw[i] = post[j0 + i * T];
  pw[P] = post[H / 2];
  const float hs = 0.5f * scale;
  constexpr bool kLinearPad = (T % 8) == 0;
  constexpr int kPadStep = T + T / 8;
  uint32_t acc[2 * P + 1] = {};
  for (int64_t r = 0; r < passes; ++r) {
    const int64_t fr = f_first + r;
    const bool live = fr < f_end;
    float2 v[8];
    // (the opaque copy of the lane index: see k_stft_mean)
    int j = j0;
    if constexpr (G::Threads > 512) asm volatile("" : "+v"(j));
    const int lp_k0 = lpad(j), lp_m0 = lpad(H - j);
    const long long base = (long long)fr * hop - (n_fft >> 1);
    const bool interior = live && base >= 0 && base + n_fft <= (long long)n;
    if (interior && n_fft == 2 * H) {
      const float* xs = x + base * x_stride;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int t0 = 2 * (j + q * T);
        const float2 w = *reinterpret_cast<const float2*>(window + t0);
        v[q] = make_float2(w.x * xs[(int64_t)t0 * x_stride], w.y * xs[(int64_t)(t0 + 1) * x_stride]);
      }
    } else if (interior) {
      const float* xs = x + base * x_stride;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int t0 = 2 * (j + q * T);
        float2 z = make_float2(0.0f, 0.0f);
        if (t0 + 1 < n_fft) {
          const float2 w = *reinterpret_cast<const float2*>(window + t0);
          z.x = w.x * xs[(int64_t)t0 * x_stride];
          z.y = w.y * xs[(int64_t)(t0 + 1) * x_stride];
        } else if (t0 < n_fft) {
          z.x = window[t0] * xs[(int64_t)t0 * x_stride];
        }
        v[q] = z;
      }
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int t0 = 2 * (j + q * T);
        float2 z = make_float2(0.0f, 0.0f);
        if (live) {
          if (t0 < n_fft) z.x = window[t0] * x[reflect_index(base + t0, n) * x_stride];
          if (t0 + 1 < n_fft) z.y = window[t0 + 1] * x[reflect_index(base + t0 + 1, n) * x_stride];
        }
        v[q] = z;
      }
    }
    // fft_core synchronises the frame's lanes before its first store to X: the previous frame's untangle reads are done by then
    fft_core<LOGH>(v, X, j, tw);
    if (live) {
      float mg[2 * P + 1];
      auto keep = [&](int s, float re, float im) { mg[s] = fmaf(__builtin_amdgcn_sqrtf(fmaf(re, re, im * im)), hs, 1e-7f); };
#pragma unroll
      for (int i = 0; i <= P; ++i) {
        const int k = (i < P) ? j + i * T : H / 2;
        if (i == P && j != 0) break;
        int sk = lpad(k), sm = lpad((H - k) & (H - 1));
        if (kLinearPad && i < P) {
          sk = lp_k0 + i * kPadStep;
          sm = (i == 0 && j == 0) ? 0 : lp_m0 - i * kPadStep;
        }
        const float2 zk = X[sk];
        const float2 zc = cconj(X[sm]);
        const float2 ev = cadd(zk, zc);
        const float2 t = cmul(pw[i], csub(zk, zc));
        keep(2 * i, ev.x + t.y, ev.y - t.x);                     // bin k
        if (i < P) keep(2 * i + 1, ev.x - t.y, -ev.y - t.x);     // bin H - k
      }
#pragma unroll
      for (int s = 0; s <= 2 * P; ++s) {
        if (s == 2 * P && j != 0) break;
        const uint32_t key = image_key(mg[s]);
        acc[s] = key > acc[s] ? key : acc[s];
      }
    }
  }
  frame_sync<T>();                                             // the last untangle reads of X are done: the slot becomes the bins' maxima
  uint32_t* D = reinterpret_cast<uint32_t*>(X);                // D[k], k <= H: 2 FrameLds words are there
#pragma unroll
  for (int i = 0; i < P; ++i) {
    D[j0 + i * T] = acc[2 * i];
    D[H - (j0 + i * T)] = acc[2 * i + 1];
  }
  if (j0 == 0) D[H / 2] = acc[2 * P];
  frame_sync<T>();
  if (!owns) return;
  // the columns of the group: col and its successors with the same range
  int64_t g_end = col + 1;
  while (g_end < width && cols[2 * g_end] == c_lo && cols[2 * g_end + 1] == c_hi) ++g_end;
  for (int r = j0; r < height; r += T) {
    int rl = rows[2 * r], rh = rows[2 * r + 1];
    rl = rl < 0 ? 0 : rl;
    rh = rh > bins ? bins : rh;
    uint32_t m = 0;
    for (int b = rl; b < rh; ++b) m = D[b] > m ? D[b] : m;
    if (n_chunks == 1) {
      for (int64_t c = col; c < g_end; ++c) peak[c * pitch + r] = __uint_as_float(m);
    } else if (m != 0) {
      for (int64_t c = col; c < g_end; ++c)
        __hip_atomic_fetch_max(reinterpret_cast<uint32_t*>(peak + c * pitch + r), m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ---- Peak / Peak Track straight from the samples (util/wow_detection.py:294-327 on the frames of util/fourier.py:37-75) --------
// One frame slot of FftGeom per traced frame frame_0 + i, i < count.  Gather, window product, transform, untangle and the
// magnitude are k_stft mode 1's expressions, operation by operation, so every value the tracker sees is the float32 that
// par_stft_f32 mode 1 would have stored for that frame (DB: its float32 dB, (float)(20 log10 of the float64 of it), what
// experiments/cyclic_wow.py:34-37 hands PeakTracker).  The untangle leaves a lane the pairs (k, H - k), k = j + i T (lane 0 also
// H/2), as documented above k_stft_mean.  Lane 0 of the slot works out the band [NL, NU) before the transform and leaves it in
// LDS beside the frames (the transform's exchanges publish it).  Behind the barrier that ends the untangle reads the lanes
// deposit the values of bins NL - 1 .. NU (and of bin bins - 1 for a band that starts on bin 0, whose left neighbour it is) into
// the frame's own LDS slot, as floats indexed by bin.  Lane j then walks bins NL + j, NL + j + T, ... upwards keeping the first
// maximum, the slot's lanes reduce (value, bin) pairs to the smaller bin on equal values -- xor butterflies inside a wave for
// T <= 64, then (T > 64) the waves' pairs through LDS -- and lane 0 finishes with peak_refine (track_band.h), the expression
// K_track evaluates on a stored spectrogram.  A NaN never wins a comparison, as in K_track's walk; a NaN on bin NL keeps bin NL.
// A slot past `count` goes along with zeros through every barrier and writes nothing.
template <int LOGH, bool UNIT>
__global__ __launch_bounds__(FftGeom<LOGH>::Threads) void k_stft_peak(const float* __restrict__ x, int64_t n, int64_t x_stride_arg,
                                                                       int n_fft, int hop, const float* __restrict__ window,
                                                                       const float2* __restrict__ tw, const float2* __restrict__ post,
                                                                       int64_t frame_0, int64_t count, double* __restrict__ freqs,
                                                                       double centre, double sr, double tol, int mode, int db,
                                                                       int* __restrict__ status, float scale) {
  const int64_t x_stride = UNIT ? 1 : x_stride_arg;
  using G = FftGeom<LOGH>;
  constexpr int H = G::H, T = G::T;
  constexpr int bins = H + 1, P = (H / 2) / T;
  constexpr int kWaves = T > kWave ? T / kWave : 1;           // waves per frame
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  const int f = threadIdx.x / T, j = threadIdx.x - f * T;
  float2* X = lds + f * G::FrameLds;
  // beside the frames: per frame the band (NL, NU, past_end, unused), then per wave of the frame one (value, bin) pair
  int* side = reinterpret_cast<int*>(lds + G::Frames * G::FrameLds) + f * (4 + 2 * kWaves);
  const int64_t slot = xcd_contiguous_block((count + G::Frames - 1) / G::Frames) * G::Frames + f;
  const bool live = slot < count;
  const int64_t fr = frame_0 + slot;
  if (j == 0) {
    Band b;
    b.NL = 0;
    b.NU = 0;
    b.past_end = false;
    if (live) b = mode == 0 ? band_limits(freqs[slot], tol, 2 * H, sr, bins) : band_limits(centre, slot > 2 ? tol / 2 : tol, 2 * H, sr, bins);
    side[0] = b.NL;
    side[1] = b.NU;
    side[2] = b.past_end ? 1 : 0;
  }
  float2 v[8];
  const long long base = (long long)fr * hop - (n_fft >> 1);
  const bool interior = live && base >= 0 && base + n_fft <= (long long)n;
  if (interior && n_fft == 2 * H) {
    const float* xs = x + base * x_stride;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int t0 = 2 * (j + q * T);
      const float2 w = *reinterpret_cast<const float2*>(window + t0);
      v[q] = make_float2(w.x * xs[(int64_t)t0 * x_stride], w.y * xs[(int64_t)(t0 + 1) * x_stride]);
    }
  } else if (interior) {
    const float* xs = x + base * x_stride;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int t0 = 2 * (j + q * T);
      float2 z = make_float2(0.0f, 0.0f);
      if (t0 + 1 < n_fft) {
        const float2 w = *reinterpret_cast<const float2*>(window + t0);
        z.x = w.x * xs[(int64_t)t0 * x_stride];
        z.y = w.y * xs[(int64_t)(t0 + 1) * x_stride];
      } else if (t0 < n_fft) {
        z.x = window[t0] * xs[(int64_t)t0 * x_stride];
      }
      v[q] = z;
    }
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int t0 = 2 * (j + q * T);
      float2 z = make_float2(0.0f, 0.0f);
      if (live) {
        if (t0 < n_fft) z.x = window[t0] * x[reflect_index(base + t0, n) * x_stride];
        if (t0 + 1 < n_fft) z.y = window[t0 + 1] * x[reflect_index(base + t0 + 1, n) * x_stride];
      }
      v[q] = z;
    }
  }
  float2 pw[P + 1];
#pragma unroll
  for (int i = 0; i < P; ++i) pw[i] = post[j + i * T];
  pw[P] = post[H / 2];
  fft_core<LOGH>(v, X, j, tw);
  const float hs = 0.5f * scale;
  constexpr bool kLinearPad = (T % 8) == 0;
  constexpr int kPadStep = T + T / 8;
  const int lp_k0 = lpad(j), lp_m0 = lpad(H - j);
  // the float32 magnitudes of this lane's bins, in registers until every lane of the frame has read X
  float mg[2 * P + 1];
  auto keep = [&](int s, float re, float im) { mg[s] = fmaf(__builtin_amdgcn_sqrtf(fmaf(re, re, im * im)), hs, 1e-7f); };
#pragma unroll
  for (int i = 0; i <= P; ++i) {
    const int k = (i < P) ? j + i * T : H / 2;
    if (i == P && j != 0) break;
    int sk = lpad(k), sm = lpad((H - k) & (H - 1));
    if (kLinearPad && i < P) {
      sk = lp_k0 + i * kPadStep;
      sm = (i == 0 && j == 0) ? 0 : lp_m0 - i * kPadStep;
    }
    const float2 zk = X[sk];
    const float2 zc = cconj(X[sm]);
    const float2 ev = cadd(zk, zc);
    const float2 t = cmul(pw[i], csub(zk, zc));
    keep(2 * i, ev.x + t.y, ev.y - t.x);                     // bin k
    if (i < P) keep(2 * i + 1, ev.x - t.y, -ev.y - t.x);     // bin H - k
  }
  frame_sync<T>();                                           // the untangle reads of X are done: the slot becomes the band's values
  Band b;
  b.NL = side[0];
  b.NU = side[1];
  b.past_end = side[2] != 0;
  const bool has_band = live && b.NL >= 0 && b.NL < b.NU;    // uniform over the frame's lanes
  float* D = reinterpret_cast<float*>(X);                    // D[k], k <= H: 2 FrameLds floats are there
  if (has_band) {
    const int lo = b.NL - 1, hi = b.NU < bins - 1 ? b.NU : bins - 1;
    auto deposit = [&](int k, float m) {
      if ((k >= lo && k <= hi) || (b.NL == 0 && k == bins - 1)) D[k] = db ? (float)(20.0 * log10_pos((double)m)) : m;
    };
#pragma unroll
    for (int i = 0; i < P; ++i) {
      deposit(j + i * T, mg[2 * i]);
      deposit(H - (j + i * T), mg[2 * i + 1]);
    }
    if (j == 0) deposit(H / 2, mg[2 * P]);
  }
  frame_sync<T>();
  float best = -INFINITY;
  int arg = 0x7fffffff;
  if (has_band) {
    for (int k = b.NL + j; k < b.NU; k += T) {
      const float val = D[k];
      if (val > best) {                                      // ascending bins per lane: strict > keeps the first occurrence
        best = val;
        arg = k;
      }
    }
  }
  constexpr int kLanes = T < kWave ? T : kWave;
#pragma unroll
  for (int o = kLanes / 2; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, kWave);
    const int oa = __shfl_xor(arg, o, kWave);
    if (ov > best || (ov == best && oa < arg)) {
      best = ov;
      arg = oa;
    }
  }
  if constexpr (T > kWave) {
    if ((j & (kWave - 1)) == 0) {
      side[4 + 2 * (j / kWave)] = __float_as_int(best);
      side[5 + 2 * (j / kWave)] = arg;
    }
    __syncthreads();
    if (j == 0) {
      for (int w = 1; w < kWaves; ++w) {
        const float ov = __int_as_float(side[4 + 2 * w]);
        const int oa = side[5 + 2 * w];
        if (ov > best || (ov == best && oa < arg)) {
          best = ov;
          arg = oa;
        }
      }
    }
  }
  if (j != 0 || !live) return;
  if (!has_band) {
    atomicOr(status, 1);
    return;
  }
  if (arg == 0x7fffffff || D[b.NL] != D[b.NL]) arg = b.NL;   // nothing but NaN, or a NaN on the first bin: K_track's walk stays on NL
  freqs[slot] = peak_refine([&](int k) { return D[k]; }, arg, b, bins, 2 * H, sr, status);
}

// ---- transforms above 8192 points: four-step FFT ----------------------------------------------------------
// The GUI offers FFT sizes up to 2^20 (util/widgets.py:333-349).  A frame of M = n_fft*zeropad real points is an
// H = M/2-point complex sequence; H = N1 N2 is transformed in two passes over HBM around the register/LDS core:
//   pass A  N2 column transforms of N1 points (input index n2 + N2 n1), times W_H^(n2 k1), stored as A[k1][n2];
//           the gather (reflect boundary), the window and the real->complex packing are fused into its loads
//   pass B  N1 row transforms of N2 points, stored at k1 + N1 k2
//   untangle to the H+1 real-FFT bins (complex, or |X| + 1e-7)
// A workgroup owns C = 8 adjacent columns (rows): both its loads and its stores then move 64-byte runs (loads and
// stores go through one LDS transposition each), and the C transforms run side by side in the core.
struct BigTw {
  float2* lo = nullptr;     // exp(-2 pi i m / H),        m = 0 .. kBigR-1
  float2* hi = nullptr;     // exp(-2 pi i m kBigR / H),  m = 0 .. H/kBigR-1
};
constexpr int kBigR = 1024;
constexpr int kBigC = 8;
static std::map<std::pair<int, int>, BigTw> g_bigtw;

static int get_big_twiddles(int device, int H, BigTw* out) {
  std::lock_guard<std::mutex> lk(g_tw_mu);
  auto key = std::make_pair(device, H);
  auto it = g_bigtw.find(key);
  if (it != g_bigtw.end()) {
    *out = it->second;
    return PAR_OK;
  }
  const int nh = H / kBigR > 1 ? H / kBigR : 1;
  std::vector<float2> lo(kBigR), hi(nh);
  for (int m = 0; m < kBigR; ++m) {
    const double a = -2.0 * M_PI * (double)m / (double)H;
    lo[m] = make_float2((float)cos(a), (float)sin(a));
  }
  for (int m = 0; m < nh; ++m) {
    const double a = -2.0 * M_PI * (double)m * (double)kBigR / (double)H;
    hi[m] = make_float2((float)cos(a), (float)sin(a));
  }
  BigTw t;
  PAR_HIP_CHECK(hipMalloc(&t.lo, lo.size() * sizeof(float2)));
  PAR_HIP_CHECK(hipMalloc(&t.hi, hi.size() * sizeof(float2)));
  PAR_HIP_CHECK(hipMemcpy(t.lo, lo.data(), lo.size() * sizeof(float2), hipMemcpyHostToDevice));
  PAR_HIP_CHECK(hipMemcpy(t.hi, hi.data(), hi.size() * sizeof(float2), hipMemcpyHostToDevice));
  g_bigtw[key] = t;
  *out = t;
  return PAR_OK;
}

// PASS 0: columns of the packed windowed frame -> A;  PASS 1: rows of A -> Z.
// grid: round_up(groups * n_batch, 8) workgroups in ONE dimension, group = kBigC adjacent transforms of one frame.  The
// hardware deals workgroups round-robin to the 8 XCDs, so neighbouring column groups -- whose 64-byte runs are the two
// halves of the same 128-byte lines, on the load and on the store side -- used to meet in eight different L2s and reach
// HBM as scattered half-line accesses (1.4 GB moved in 0.79 ms).  xcd_contiguous_block() hands every XCD a contiguous
// range of (frame, group) pairs instead, so the halves merge in one L2.
__host__ __device__ constexpr int64_t round_up8(int64_t v) { return (v + 7) & ~7ll; }
template <int LOGS, int PASS, int SRC = 0>
__global__ __launch_bounds__(1 << LOGS) void k_bigfft(const float* __restrict__ x, int64_t n, int64_t x_stride, int n_fft, int hop,
                                                      const float* __restrict__ window, const float2* __restrict__ tw,
                                                      const float2* __restrict__ tlo, const float2* __restrict__ thi,
                                                      float2* __restrict__ A, float2* __restrict__ Z, int64_t f_first,
                                                      int logN1, int logN2, int64_t n_batch) {
  static_assert(LOGS >= 6 && LOGS <= 10, "one lane per 8 points, kBigC transforms side by side: blockDim.x == 1 << LOGS");
  constexpr int S = 1 << LOGS, T = S / 8;
  constexpr int FrameLds = S + S / 8 + 8;
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  const int N1 = 1 << logN1, N2 = 1 << logN2;
  const int64_t H = (int64_t)N1 * N2;
  const int tid = threadIdx.x;
  const int groups = (PASS == 0 ? N2 : N1) / kBigC;
  const int64_t w = xcd_contiguous_block(groups * n_batch);
  if (w >= groups * n_batch) return;
  const int64_t fb = w / groups;                           // frame of this batch
  const int g0 = (int)(w - fb * groups) * kBigC;           // first column (pass 0) / row (pass 1) of the group
  float2* Ab = A + fb * H;
  // every loop below runs kBigC times with compile-time bounds: all of a thread's loads are in flight together
  if (PASS == 0 && SRC == 1) {                             // plain complex input, transformed in place
#pragma unroll
    for (int it = 0; it < kBigC; ++it) {
      const int idx = tid + it * S, n1 = idx / kBigC, f = idx % kBigC;
      lds[f * FrameLds + lpad(n1)] = Ab[(int64_t)(g0 + f) + (int64_t)N2 * n1];
    }
  } else if (PASS == 0) {
    const long long base = (long long)(f_first + fb) * hop - (n_fft >> 1);
    // a frame that lies inside the signal (all but the first and last few) indexes it directly; the reflect fold is a
    // 64-bit modulo per sample
    if (base >= 0 && base + n_fft <= (long long)n) {
      const float* xs = x + base * x_stride;
      // contiguous signal, frame starting on an 8-byte boundary (even hop and n_fft / 2): the two samples of a packed
      // point arrive in one load
      const bool paired = x_stride == 1 && (reinterpret_cast<uintptr_t>(xs) & 7) == 0;
      // branch-free: n_fft is even, so a packed pair lies entirely inside the frame or entirely in the zero padding; a
      // padded pair loads the frame's last pair instead and is zeroed afterwards (a branch per pair made every load wait
      // for the one before it)
      float2 z[kBigC], wv[kBigC];
      int t0[kBigC];
#pragma unroll
      for (int it = 0; it < kBigC; ++it) {
        const int idx = tid + it * S, n1 = idx / kBigC, f = idx % kBigC;
        t0[it] = 2 * (g0 + f + N2 * n1);                   // first real sample of the packed pair (< n_fft * zeropad <= 2^21)
        const int tc = t0[it] < n_fft ? t0[it] : n_fft - 2;
        wv[it] = *reinterpret_cast<const float2*>(window + tc);
        t0[it] = t0[it] < n_fft ? tc : -1;
      }
      if (paired) {
#pragma unroll
        for (int it = 0; it < kBigC; ++it) z[it] = *reinterpret_cast<const float2*>(xs + (t0[it] < 0 ? n_fft - 2 : t0[it]));
      } else {
#pragma unroll
        for (int it = 0; it < kBigC; ++it) {
          const int64_t tc = t0[it] < 0 ? n_fft - 2 : t0[it];
          z[it] = make_float2(xs[tc * x_stride], xs[(tc + 1) * x_stride]);
        }
      }
#pragma unroll
      for (int it = 0; it < kBigC; ++it) {
        z[it].x = t0[it] < 0 ? 0.0f : wv[it].x * z[it].x;
        z[it].y = t0[it] < 0 ? 0.0f : wv[it].y * z[it].y;
      }
#pragma unroll
      for (int it = 0; it < kBigC; ++it) {
        const int idx = tid + it * S, n1 = idx / kBigC, f = idx % kBigC;
        lds[f * FrameLds + lpad(n1)] = z[it];
      }
    } else {
      for (int it = 0; it < kBigC; ++it) {
        const int idx = tid + it * S, n1 = idx / kBigC, f = idx % kBigC;
        const long long t0 = 2ll * ((long long)(g0 + f) + (long long)N2 * n1);
        float2 z = make_float2(0.0f, 0.0f);
        if (t0 < n_fft) z.x = window[t0] * x[reflect_index(base + t0, n) * x_stride];
        if (t0 + 1 < n_fft) z.y = window[t0 + 1] * x[reflect_index(base + t0 + 1, n) * x_stride];
        lds[f * FrameLds + lpad(n1)] = z;
      }
    }
  } else {
#pragma unroll
    for (int f = 0; f < kBigC; ++f) lds[f * FrameLds + lpad(tid)] = Ab[(int64_t)(g0 + f) * N2 + tid];
  }
  __syncthreads();
  // kBigC transforms side by side: thread -> (transform f, lane j)
  const int f = tid / T, j = tid - f * T;
  float2* X = lds + f * FrameLds;
  float2 v[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) v[q] = X[lpad(j + q * T)];
  fft_core<LOGS>(v, X, j, tw);
  __syncthreads();
  if (PASS == 0) {
    float2 wv[kBigC];
#pragma unroll
    for (int it = 0; it < kBigC; ++it) {
      const int idx = tid + it * S, k1 = idx / kBigC, ff = idx % kBigC;
      const unsigned m = (unsigned)(g0 + ff) * (unsigned)k1;       // < H <= 2^20
      wv[it] = cmul(thi[m / kBigR], tlo[m % kBigR]);
    }
#pragma unroll
    for (int it = 0; it < kBigC; ++it) {
      const int idx = tid + it * S, k1 = idx / kBigC, ff = idx % kBigC;
      Ab[(int64_t)k1 * N2 + g0 + ff] = cmul(lds[ff * FrameLds + lpad(k1)], wv[it]);
    }
  } else {
    float2* Zb = Z + fb * H;
#pragma unroll
    for (int it = 0; it < kBigC; ++it) {
      const int idx = tid + it * S, k2 = idx / kBigC, ff = idx % kBigC;
      Zb[(int64_t)(g0 + ff) + (int64_t)N1 * k2] = lds[ff * FrameLds + lpad(k2)];
    }
  }
}

// Row pass of the STFT, fused with the untangle to the H+1 real-FFT bins
//   X[k] = (Z[k] + conj Z[H-k])/2 - i W_2H^k (Z[k] - conj Z[H-k])/2,      k = k1 + N1 k2,  H - k = (N1 - k1) + N1 (N2 - 1 - k2):
// a bin's partner lives in row N1 - k1, so a workgroup transforms the kBigC rows k1 = 8m+1 .. 8m+8 AND their partners
// N1-8m-8 .. N1-8m-1 (two rounds through the core, all 16 spectra staying in LDS) and writes both output runs itself:
// the H-point spectrum Z never travels to HBM (it used to be written, then read back by a separate untangle kernel:
// 2 x 8 H bytes per frame of the pass's 3 x 8 H).  Row N1/2 pairs with itself and rides on both sides of the last
// regular group; row 0 pairs with itself under k2 -> (N2 - k2) mod N2 and has the extra group blockIdx.x == N1/16.
// tlo2/thi2: the two-level table of the 2H-point circle.  MODE 0: complex bins, 1: |X| + 1e-7.
template <int LOGS, int MODE>
__global__ __launch_bounds__(1 << LOGS) void k_bigfft_rows_out(const float2* __restrict__ A, const float2* __restrict__ tw,
                                                               const float2* __restrict__ tlo2, const float2* __restrict__ thi2,
                                                               float* __restrict__ out, int64_t f_first, int logN1, float scale,
                                                               int64_t n_batch) {
  static_assert(LOGS >= 6 && LOGS <= 10, "one lane per 8 points, 8 transforms per round");
  constexpr int S = 1 << LOGS, T = S / 8, N2 = S;
  constexpr int FrameLds = S + S / 8 + 8;
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  const int N1 = 1 << logN1;
  const int64_t H = (int64_t)N1 * N2, bins = H + 1;
  const int tid = threadIdx.x;                               // blockDim.x == S
  // one grid dimension, XCD-contiguous like k_bigfft: neighbouring groups write neighbouring 32/64-byte runs
  const int groups = N1 / (2 * kBigC) + 1;
  const int64_t w = xcd_contiguous_block(groups * n_batch);
  if (w >= groups * n_batch) return;
  const int64_t fb = w / groups, fr = f_first + fb;
  const float2* Ab = A + fb * H;
  const int m = (int)(w - fb * groups);
  const bool row0 = m == N1 / 16;
  const int p0 = 8 * m + 1, q0 = N1 - 8 * m - 8;             // first row of the group, first row of its partners
  if (row0) {
    lds[lpad(tid)] = Ab[tid];
#pragma unroll
    for (int f = 1; f < kBigC; ++f) lds[f * FrameLds + lpad(tid)] = make_float2(0.0f, 0.0f);
  } else {
#pragma unroll
    for (int f = 0; f < 2 * kBigC; ++f) {
      const int row = f < kBigC ? p0 + f : q0 + (f - kBigC);
      lds[f * FrameLds + lpad(tid)] = Ab[(int64_t)row * N2 + tid];
    }
  }
  __syncthreads();
  const int f = tid / T, j = tid - f * T;
  for (int round = 0; round < (row0 ? 1 : 2); ++round) {
    float2* X = lds + (round * kBigC + f) * FrameLds;
    float2 v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = X[lpad(j + q * T)];
    fft_core<LOGS>(v, X, j, tw);
  }
  __syncthreads();
  const float hs = 0.5f * scale;
  auto emit = [&](int64_t kk, float re, float im) {
    // plain stores: a group's runs are 32 (magnitudes) or 64 bytes long and complete their 128-byte lines only together with
    // the neighbouring groups' -- in L2.  Streaming (nontemporal) stores, right for K_stft's whole rows, sent every run to
    // HBM on its own: 0.85 ms for this kernel against 0.32 ms (0.25 ms with the stores removed altogether).
    if constexpr (MODE == 0) reinterpret_cast<float2*>(out)[fr * bins + kk] = make_float2(re * hs, im * hs);
    else out[fr * bins + kk] = fmaf(__builtin_amdgcn_sqrtf(fmaf(re, re, im * im)), hs, 1e-7f);
  };
  auto half_step = [&](int64_t k) { return cmul(thi2[(uint64_t)k / kBigR], tlo2[(uint64_t)k % kBigR]); };
  if (row0) {
    if (tid <= N2 / 2) {
      const int k2 = tid;
      const int64_t k = (int64_t)N1 * k2;
      const float2 zk = lds[lpad(k2)];
      const float2 zc = cconj(lds[lpad((N2 - k2) & (N2 - 1))]);
      const float2 ev = cadd(zk, zc);
      const float2 t = cmul(half_step(k), csub(zk, zc));
      emit(k, ev.x + t.y, ev.y - t.x);
      if (k2 > 0 && k2 < N2 / 2) emit(H - k, ev.x - t.y, -ev.y - t.x);
      if (k2 == 0) emit(H, ev.x - t.y, -ev.y - t.x);
    }
    return;
  }
#pragma unroll
  for (int it = 0; it < kBigC; ++it) {
    const int idx = tid + it * S;
    const int k2 = idx / kBigC, i = idx % kBigC;
    const int k1 = p0 + i;
    if (k1 == N1 / 2 && k2 >= N2 / 2) continue;              // the self-paired row: each pair once
    const int64_t k = k1 + (int64_t)N1 * k2;
    const float2 zk = lds[i * FrameLds + lpad(k2)];
    const float2 zc = cconj(lds[(2 * kBigC - 1 - i) * FrameLds + lpad(N2 - 1 - k2)]);
    const float2 ev = cadd(zk, zc);
    const float2 t = cmul(half_step(k), csub(zk, zc));
    emit(k, ev.x + t.y, ev.y - t.x);
    emit(H - k, ev.x - t.y, -ev.y - t.x);
  }
}

// H-point complex FFT (H a power of two in [8192, 2^20]) of `batch` arrays: A is overwritten, the spectrum lands in Z
static int big_fft_c2c(int device, float2* A, float2* Z, int64_t H, int64_t batch, hipStream_t s) {
  const int L = [&] { int l = 0; while ((1ll << l) < H) ++l; return l; }(), l1 = (L + 1) / 2, l2 = L - l1;
  PAR_REQUIRE(H >= 8192 && H <= (1ll << 20) && (1ll << L) == H, PAR_ERR_UNSUPPORTED, "big_fft_c2c: H=%lld", (long long)H);
  Twiddles t1, t2;
  BigTw bt;
  int rc = get_twiddles(device, 2 << l1, &t1);
  if (rc == PAR_OK) rc = get_twiddles(device, 2 << l2, &t2);
  if (rc == PAR_OK) rc = get_big_twiddles(device, (int)H, &bt);
  if (rc != PAR_OK) return rc;
#define PAR_BIG_C2C(LS, PASS, NG, TW)                                                                                     \
  if (int rc_lds = raise_dynamic_lds(reinterpret_cast<const void*>(&k_bigfft<LS, PASS, 1>),                               \
                                     kBigC * ((1 << LS) + (1 << LS) / 8 + 8) * (int)sizeof(float2), device))              \
    return rc_lds;                                                                                                        \
  hipLaunchKernelGGL((k_bigfft<LS, PASS, 1>), dim3((unsigned)round_up8((int64_t)((NG) / kBigC) * batch)), dim3(1 << LS),   \
                     (size_t)kBigC * ((1 << LS) + (1 << LS) / 8 + 8) * sizeof(float2), s, (const float*)nullptr, (int64_t)0, \
                     (int64_t)1, 0, 1, (const float*)nullptr, TW, bt.lo, bt.hi, A, Z, (int64_t)0, l1, l2, batch)
  switch (l1) {
    case 7: PAR_BIG_C2C(7, 0, 1 << l2, t1.w); break;
    case 8: PAR_BIG_C2C(8, 0, 1 << l2, t1.w); break;
    case 9: PAR_BIG_C2C(9, 0, 1 << l2, t1.w); break;
    case 10: PAR_BIG_C2C(10, 0, 1 << l2, t1.w); break;
    default: PAR_REQUIRE(false, PAR_ERR_UNSUPPORTED, "big_fft_c2c: unsupported size");
  }
  switch (l2) {
    case 6: PAR_BIG_C2C(6, 1, 1 << l1, t2.w); break;
    case 7: PAR_BIG_C2C(7, 1, 1 << l1, t2.w); break;
    case 8: PAR_BIG_C2C(8, 1, 1 << l1, t2.w); break;
    case 9: PAR_BIG_C2C(9, 1, 1 << l1, t2.w); break;
    case 10: PAR_BIG_C2C(10, 1, 1 << l1, t2.w); break;
    default: PAR_REQUIRE(false, PAR_ERR_UNSUPPORTED, "big_fft_c2c: unsupported size");
  }
#undef PAR_BIG_C2C
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}

// ---- transforms of 2^22 .. 2^24 points (r03): one more radix step around the four-step transform ------------------------
// The GUI offers FFT sizes to 2^20 with zero-padding to 16 (util/widgets.py:334-351): frames of up to 2^24 real points, an
// H = 2^23-point complex sequence z.  The four-step core holds rows / columns of <= 1024 points (H <= 2^20), so the
// sequence is decimated in time by R = H / 2^20 (2, 4 or 8): z_r[m] = z[R m + r] are R sequences of 2^20 points,
// transformed as a batch by big_fft_c2c, and
//     Z[k' + H' q] = sum_r W_R^(r q) (W_H^(r k') Z_r[k'])          k' < H' = 2^20, q < R
// is formed bin by bin in the kernel that also untangles the real transform and writes |X| or X.  Five passes over an
// H-point array per frame instead of the four-step's three, for sizes the reference's CPU chain needs seconds per frame for.
//   k_huge_gather   z_r[m] = (xw[2 (R m + r)], xw[2 (R m + r) + 1]): window, reflect boundary, zero padding
//   k_huge_out      R-point recombination with float64 twiddles, untangle, magnitude
__global__ __launch_bounds__(256) void k_huge_gather(const float* __restrict__ x, int64_t n, int64_t x_stride, int n_fft, int hop,
                                                     const float* __restrict__ window, int64_t frame, int logR, int64_t Hp,
                                                     float2* __restrict__ z) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;        // t = r Hp + m
  if (t >= (Hp << logR)) return;
  const int64_t r = t / Hp, m = t - r * Hp;
  const int64_t i = (m << logR) + r;                                        // packed point of the frame
  const long long base = (long long)frame * hop - (n_fft >> 1);
  float2 v = make_float2(0.0f, 0.0f);
  const int64_t t0 = 2 * i;
  if (t0 < n_fft) v.x = window[t0] * x[reflect_index(base + t0, n) * x_stride];
  if (t0 + 1 < n_fft) v.y = window[t0 + 1] * x[reflect_index(base + t0 + 1, n) * x_stride];
  z[t] = v;
}

template <int MODE>
__global__ __launch_bounds__(256) void k_huge_out(const float2* __restrict__ Zr, int logR, int64_t Hp, float* __restrict__ out,
                                                  int64_t row, float scale) {
  const int64_t kp = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;       // k' < H'
  if (kp >= Hp) return;
  const int R = 1 << logR;
  const int64_t H = Hp << logR;
  // the R bins k' + H' q of this thread and their partners H - k = (H' - k') + H' (R - 1 - q)  (k' = 0: H' ((R - q) mod R))
  const int64_t kc = kp == 0 ? 0 : Hp - kp;
  double ar[8], ai[8], br[8], bi[8];                                        // W_H^(r k') Z_r[k'] and the same at k'' = kc
  double s1, c1, s2, c2;
  sincospi(-2.0 * (double)kp / (double)H, &s1, &c1);
  sincospi(-2.0 * (double)kc / (double)H, &s2, &c2);
  double w1r = 1.0, w1i = 0.0, w2r = 1.0, w2i = 0.0;
  for (int r = 0; r < R; ++r) {
    const float2 a = Zr[(int64_t)r * Hp + kp], b = Zr[(int64_t)r * Hp + kc];
    ar[r] = (double)a.x * w1r - (double)a.y * w1i;
    ai[r] = (double)a.x * w1i + (double)a.y * w1r;
    br[r] = (double)b.x * w2r - (double)b.y * w2i;
    bi[r] = (double)b.x * w2i + (double)b.y * w2r;
    const double t1 = w1r * c1 - w1i * s1, t2 = w2r * c2 - w2i * s2;
    w1i = w1r * s1 + w1i * c1;
    w1r = t1;
    w2i = w2r * s2 + w2i * c2;
    w2r = t2;
  }
  const double hs = 0.5 * (double)scale;
  for (int q = 0; q < R; ++q) {
    const int qp = kp == 0 ? (R - q) & (R - 1) : R - 1 - q;                // the partner's q
    double zr = 0.0, zi = 0.0, pr = 0.0, pi_ = 0.0;
    for (int r = 0; r < R; ++r) {                                           // W_R^(r q): exact multiples of 1/R turns
      double sq, cq, sp, cp;
      sincospi(-2.0 * (double)((r * q) & (R - 1)) / (double)R, &sq, &cq);
      sincospi(-2.0 * (double)((r * qp) & (R - 1)) / (double)R, &sp, &cp);
      zr += ar[r] * cq - ai[r] * sq;
      zi += ar[r] * sq + ai[r] * cq;
      pr += br[r] * cp - bi[r] * sp;
      pi_ += br[r] * sp + bi[r] * cp;
    }
    // X[k] = (Z[k] + conj Z[H-k])/2 - i W_2H^k (Z[k] - conj Z[H-k])/2
    const int64_t k = kp + Hp * q;
    double sk, ck;
    sincospi(-(double)k / (double)H, &sk, &ck);
    const double evr = zr + pr, evi = zi - pi_, dr = zr - pr, di = zi + pi_;
    const double tr = ck * dr - sk * di, ti = ck * di + sk * dr;            // W^k (Z[k] - conj Z[H-k])
    const double xr = (evr + ti) * hs, xi = (evi - tr) * hs;
    if (MODE == 0) reinterpret_cast<float2*>(out)[row + k] = make_float2((float)xr, (float)xi);
    else out[row + k] = (float)(sqrt(xr * xr + xi * xi) + 1e-7);
    if (k == 0) {                                                           // bin H: X[H] = Re Z[0] - Im Z[0]
      const double xh = (zr - zi) * 2.0 * hs;
      if (MODE == 0) reinterpret_cast<float2*>(out)[row + H] = make_float2((float)xh, 0.0f);
      else out[row + H] = (float)(fabs(xh) + 1e-7);
    }
  }
}

// ---- X2: normalised cross-correlation and delay search (util/correlation.py:6-39) ---------------------------
// scipy.signal.correlate(a/|a|, b/|b|, 'full') through ONE complex transform of z = a + i b (both zero-padded to
// N >= len a + len b - 1): A_k = (Z_k + conj Z_{N-k})/2, B_k = (Z_k - conj Z_{N-k})/(2i), cross spectrum A conj(B),
// inverse transform by the conjugate trick.  z is packed from the NORMALISED signals: each half of Z_k carries the float32
// rounding of the whole of z, so with the raw signals a take 40 dB below the other one came out 100 times less exact
// (tests/test_xcorr_gpu.py, unequal levels).  The float32 transform places the peak (error ~1e-6 of it); find_delay
// then re-evaluates the few lags around it as float64 dot products, so the parabola through the peak -- the delay
// the tape-sync tool uses -- is exact.
// ONE family of kernels (k_xcb_*) serves a batch of W pairs of rows of one shape (pytapesynch_gui.py:210-238, the azimuth
// mode) and the single pair, which is the batch of one: every rule of the search -- the first maximum, the rival list, the
// plateau, the tie, the best of five, the f[-1] wrap, the last-lag status, the parabola -- is written once, on the device,
// and no value travels to the host between the stages.  Only k_xc_unpack / k_xc_unpack_acc are the single pair's own: the
// float64 'full' array is par_xcorr_f64's product, the sectioned form's accumulator and what the single pair's peak stage scans.
// full[j] = circ[(j - (nb-1)) mod N] / N, j = 0 .. na + nb - 2 (the signals went in normalised)
__global__ __launch_bounds__(256) void k_xc_unpack(const float2* __restrict__ Y, int64_t N, int64_t nb, int64_t n_full,
                                                   double* __restrict__ full) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_full) return;
  full[j] = (double)Y[(j - (nb - 1)) & (N - 1)].x / (double)N;
}
// sectioned form: full[j] += circ[(j - (nbq-1)) mod N] / N for the n_local lags of one section pair
__global__ __launch_bounds__(256) void k_xc_unpack_acc(const float2* __restrict__ Y, int64_t N, int64_t nbq, int64_t n_local,
                                                       double* __restrict__ full) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_local) return;
  full[j] += (double)Y[(j - (nbq - 1)) & (N - 1)].x / (double)N;
}
// |v| in float64 by one 1024-thread workgroup (valid in thread 0): THE summation order of the norm
__device__ inline double xc_norm_1024(const double* __restrict__ v, int64_t n, double* part /* LDS [16] */) {
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 1024) acc += v[i] * v[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, kWave);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) {
    for (int w = 0; w < 16; ++w) t += part[w];
    t = sqrt(t);
  }
  return t;
}
constexpr int kXcCand = 64;                        // rival peaks find_delay re-evaluates exactly
// Listing tolerance: a rival is listed when the transform puts it within kXcRivalTol of the transform's top.  With e the
// transform's worst error, a rival whose exact value reaches the exact top reads at least top - 2e, so 2e <= kXcRivalTol
// lists it for certain (include/par_hip.h; measured per transform size in tests/test_xcorr_gpu.py, NOTES.md "Correlation").
constexpr double kXcRivalTol = 4.0e-6;
// exact 'same' correlation value at lag j by one 256-thread workgroup (valid in thread 0), float64:
// same[j] = sum_t a[t + j + (nb-1)//2 - (nb-1)] b[t] / (|a| |b|).  THE summation order of every value that enters a delay.
__device__ inline double xc_exact_256(const double* __restrict__ a, int64_t na, const double* __restrict__ b, int64_t nb,
                                      const double* __restrict__ norms, int64_t j, double* part /* LDS [4] */) {
  double acc = 0.0;
  if (j >= 0 && j < na) {
    const int64_t sh = j + (nb - 1) / 2 - (nb - 1);
    for (int64_t t = threadIdx.x; t < nb; t += 256) {
      const int64_t ia = t + sh;
      if (ia >= 0 && ia < na) acc += a[ia] * b[t];
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, kWave);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  return threadIdx.x == 0 ? (part[0] + part[1] + part[2] + part[3]) / (norms[0] * norms[1]) : 0.0;
}

// Per row w (a window of the batch; the single pair is row 0) the tables in scratch are XcbRow: norms, the transform's top,
// the rival list and its exact values, the seven exact values around the peak and the f[-1] wrap.  In every kernel below
// the grid's y extent (or, one thread or workgroup per row, its x extent) runs over the rows.
struct XcbRow {
  double norms[2];
  long long arg;
  int n_cand, pad;
  long long cand[kXcCand + 1];
  double cvals[kXcCand + 1];
  double vals[8];                                  // lags arg-3 .. arg+3, and lag na-1 (numpy's f[-1] at peak 0)
};
// rows *= window, in place like util/correlation.py:18-20 (grid: x over samples, y over windows)
__global__ __launch_bounds__(256) void k_xcb_window(double* __restrict__ a, int64_t a_pitch, int64_t na, double* __restrict__ b,
                                                    int64_t b_pitch, int64_t nb, const double* __restrict__ win_a,
                                                    const double* __restrict__ win_b) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, w = blockIdx.y;
  if (win_a && i < na) a[w * a_pitch + i] *= win_a[i];
  if (win_b && i < nb) b[w * b_pitch + i] *= win_b[i];
}
// norms[0] = |a|, norms[1] = |b| of every row (float64, one workgroup each)
__global__ __launch_bounds__(1024) void k_xcb_norms(const double* __restrict__ a, int64_t a_pitch, int64_t na,
                                                    const double* __restrict__ b, int64_t b_pitch, int64_t nb,
                                                    XcbRow* __restrict__ rows) {
  __shared__ double part[16];
  const int64_t w = blockIdx.y;
  const double t = xc_norm_1024(blockIdx.x ? b + w * b_pitch : a + w * a_pitch, blockIdx.x ? nb : na, part);
  if (threadIdx.x == 0) rows[w].norms[blockIdx.x] = t;
}
// z = a/|a| + i b/|b|, zero-padded to N, row by row (the sectioned form packs na, nb samples of a section pair and divides
// by the norms of the whole signals)
__global__ __launch_bounds__(256) void k_xcb_pack(const double* __restrict__ a, int64_t a_pitch, int64_t na,
                                                  const double* __restrict__ b, int64_t b_pitch, int64_t nb,
                                                  const XcbRow* __restrict__ rows, float2* __restrict__ Z, int64_t N) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, w = blockIdx.y;
  if (i >= N) return;
  const double* ar = a + w * a_pitch;
  const double* br = b + w * b_pitch;
  Z[w * N + i] = make_float2(i < na ? (float)(ar[i] / rows[w].norms[0]) : 0.0f, i < nb ? (float)(br[i] / rows[w].norms[1]) : 0.0f);
}
// conj(A_k conj(B_k)) for the second (forward) transform
__global__ __launch_bounds__(256) void k_xcb_cross(const float2* __restrict__ Z, float2* __restrict__ C, int64_t N) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x, w = blockIdx.y;
  if (k >= N) return;
  const float2 zk = Z[w * N + k], zc = cconj(Z[w * N + ((N - k) & (N - 1))]);
  const float2 A = make_float2(0.5f * (zk.x + zc.x), 0.5f * (zk.y + zc.y));
  const float2 d = csub(zk, zc);                            // 2i B_k  ->  B_k = (d.y, -d.x)/2
  const float2 B = make_float2(0.5f * d.y, -0.5f * d.x);
  const float2 c = cmul(A, cconj(B));
  C[w * N + k] = cconj(c);
}
// Where the peak stage reads lag j of row w's 'same' span.  XcLagsOfY: straight out of the second transform's output --
// full[j] = (double)Y[(j - (nb-1)) mod N].x / N is formed value by value and never stored (the rows of a batch).
// XcLagsOfFull: the float64 'full' array of ONE row, the same doubles stored (the single pair).
struct XcLagsOfY {
  const float2* __restrict__ Y;
  int64_t N;
  __device__ auto row(int64_t w, int64_t nb) const {
    const float2* Yw = Y + w * N;
    const int64_t n = N, off = (nb - 1) / 2 - (nb - 1);
    const double dN = (double)N;
    return [=](int64_t j) { return (double)Yw[(j + off) & (n - 1)].x / dN; };
  }
};
struct XcLagsOfFull {
  const double* __restrict__ full;
  __device__ auto row(int64_t, int64_t nb) const {
    const double* same_span = full + (nb - 1) / 2;
    return [=](int64_t j) { return same_span[j]; };
  }
};
// One workgroup of T threads per row: the first index of the maximum of the 'same' span (of its magnitude under use_abs),
// then the rival list in LDS.  Rival peaks: the float32 transform finds the peak to ~1e-6 of its height; a
// periodic tone, or the +/- lobes under ignore_phase, can put another local maximum within that distance of the top more
// than two lags away, and the reference's float64 argmax may pick that one.  Every local maximum within `tol` of the
// transform's top, more than two lags from it, is listed (up to kXcCand of them) for exact re-evaluation.  Nothing here
// depends on T: the reduction keeps the lowest index of the maximum, and the list is a set that k_xcb_decide orders by
// (value, lag).  T is 256 beside the other rows of a batch, 1024 where one workgroup scans up to 2^26 lags.
template <class Lags, int T>
__global__ __launch_bounds__(T) void k_xcb_peak(Lags src, int64_t na, int64_t nb, int use_abs, double tol, XcbRow* __restrict__ rows) {
  __shared__ double bv[T];
  __shared__ long long bi[T];
  __shared__ long long lcand[kXcCand];
  __shared__ int lcount;
  const int64_t w = blockIdx.x;
  const auto lag = src.row(w, nb);
  auto same = [&](int64_t j) {
    const double x = lag(j);
    return use_abs ? fabs(x) : x;
  };
  double best = -INFINITY;
  long long at = 0;
  for (int64_t i = threadIdx.x; i < na; i += T) {
    const double x = same(i);
    if (x > best) {
      best = x;
      at = i;
    }
  }
  bv[threadIdx.x] = best;
  bi[threadIdx.x] = at;
  if (threadIdx.x == 0) lcount = 0;
  __syncthreads();
  for (int o = T / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      const double x = bv[threadIdx.x + o];
      const long long j = bi[threadIdx.x + o];
      if (x > bv[threadIdx.x] || (x == bv[threadIdx.x] && j < bi[threadIdx.x])) {
        bv[threadIdx.x] = x;
        bi[threadIdx.x] = j;
      }
    }
    __syncthreads();
  }
  const long long top = bi[0];
  const double m = same(top);
  for (int64_t i = threadIdx.x; i < na; i += T) {
    if (i >= top - 2 && i <= top + 2) continue;
    const double x = same(i);
    if (!(x >= m - tol)) continue;
    const double xl = i > 0 ? same(i - 1) : -INFINITY;
    const double xr = i + 1 < na ? same(i + 1) : -INFINITY;
    if (x >= xl && x >= xr) {
      const int slot = atomicAdd(&lcount, 1);
      if (slot < kXcCand) lcand[slot] = i;
    }
  }
  __syncthreads();
  const int nc = lcount;
  XcbRow& r = rows[w];
  if (nc > 0 && nc < kXcCand) {                    // as many rivals as slots or more: a plateau, the transform's top stands
    if (threadIdx.x < nc) r.cand[threadIdx.x] = lcand[threadIdx.x];
    if (threadIdx.x == 0) r.cand[nc] = top;       // the top goes into slot nc
  }
  if (threadIdx.x == 0) {
    r.arg = top;
    r.n_cand = nc;
  }
}
// exact values of the listed rivals and the top: grid (kXcCand, windows), entries behind the list return at once
__global__ __launch_bounds__(256) void k_xcb_exact_list(const double* __restrict__ a, int64_t a_pitch, int64_t na,
                                                        const double* __restrict__ b, int64_t b_pitch, int64_t nb,
                                                        XcbRow* __restrict__ rows) {
  __shared__ double part[4];
  const int64_t w = blockIdx.y;
  XcbRow& r = rows[w];
  const int nc = r.n_cand;
  if (!(nc > 0 && nc < kXcCand) || (int)blockIdx.x > nc) return;
  const double v = xc_exact_256(a + w * a_pitch, na, b + w * b_pitch, nb, r.norms, r.cand[blockIdx.x], part);
  if (threadIdx.x == 0) r.cvals[blockIdx.x] = v;
}
// the exact values decide, the lowest lag wins a tie (np.argmax returns the first maximum): one thread per window
__global__ __launch_bounds__(64) void k_xcb_decide(XcbRow* __restrict__ rows, int64_t count, int use_abs) {
  const int64_t w = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (w >= count) return;
  XcbRow& r = rows[w];
  const int nc = r.n_cand;
  if (!(nc > 0 && nc < kXcCand)) return;
  int best = nc;
  for (int c = 0; c < nc; ++c) {
    const double x = use_abs ? fabs(r.cvals[c]) : r.cvals[c], y = use_abs ? fabs(r.cvals[best]) : r.cvals[best];
    if (x > y || (x == y && r.cand[c] < r.cand[best])) best = c;
  }
  r.arg = r.cand[best];
}
// exact values at arg-3 .. arg+3 (blockIdx.x 0 .. 6) and, where the final peak can be lag 0 (arg <= 2), at lag na-1
__global__ __launch_bounds__(256) void k_xcb_exact7(const double* __restrict__ a, int64_t a_pitch, int64_t na,
                                                    const double* __restrict__ b, int64_t b_pitch, int64_t nb,
                                                    XcbRow* __restrict__ rows) {
  __shared__ double part[4];
  const int64_t w = blockIdx.y;
  XcbRow& r = rows[w];
  const long long p0 = r.arg;
  if (blockIdx.x == 7 && p0 > 2) return;
  const int64_t j = blockIdx.x == 7 ? na - 1 : p0 - 3 + (int64_t)blockIdx.x;
  const double v = xc_exact_256(a + w * a_pitch, na, b + w * b_pitch, nb, r.norms, j, part);
  if (threadIdx.x == 0) r.vals[blockIdx.x] = v;
}
// best of arg-2 .. arg+2, the status and parabolic() (util/correlation.py:42-46), one thread per row.  The arithmetic is
// numpy's float64, rounding by rounding (f[-1] wraps to the last lag at peak 0): no contraction into FMAs here.
__global__ __launch_bounds__(64) void k_xcb_final(const XcbRow* __restrict__ rows, int64_t count, int64_t na, int use_abs,
                                                  double* __restrict__ delay, double* __restrict__ corr, int32_t* __restrict__ status) {
#pragma clang fp contract(off)
  const int64_t w = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (w >= count) return;
  const XcbRow& r = rows[w];
  const long long p0 = r.arg;
  const double* v = r.vals;
  int best = 3;
  for (int c = 1; c <= 5; ++c) {
    const long long j = p0 - 3 + c;
    if (j < 0 || j >= na) continue;
    const double x = use_abs ? fabs(v[c]) : v[c], y = use_abs ? fabs(v[best]) : v[best];
    if (x > y || (x == y && c < best)) best = c;
  }
  const long long peak = p0 - 3 + best;
  if (peak == na - 1) {                              // the reference's IndexError in parabolic(), for this row only
    delay[w] = NAN;
    corr[w] = NAN;
    status[w] = 1;
    return;
  }
  const double fm = peak == 0 ? v[7] : v[best - 1], f0 = v[best], fp = v[best + 1];
  const double xv = 0.5 * (fm - fp) / (fm - 2.0 * f0 + fp) + (double)peak;
  corr[w] = f0 - 0.25 * (fm - fp) * (xv - (double)peak);
  delay[w] = xv - (double)(na / 2);
  status[w] = 0;
}
// The delay search of c rows from their lags on (`lags`: the transforms' output, or the one row's 'full' array): peak and
// rival list -> exact values of the listed lags -> the decision -> seven exact values and the wrap -> delay, corr and
// status per row.  Everything is decided on the device; nothing here waits for it.
template <class Lags, int T>
static void xc_search(Lags lags, const double* a, int64_t a_pitch, int64_t na, const double* b, int64_t b_pitch, int64_t nb,
                      int64_t c, int ignore_phase, XcbRow* rows, double* delay, double* corr, int32_t* status, hipStream_t s) {
  hipLaunchKernelGGL((k_xcb_peak<Lags, T>), dim3((unsigned)c), dim3(T), 0, s, lags, na, nb, ignore_phase, kXcRivalTol, rows);
  hipLaunchKernelGGL(k_xcb_exact_list, dim3(kXcCand, (unsigned)c), dim3(256), 0, s, a, a_pitch, na, b, b_pitch, nb, rows);
  hipLaunchKernelGGL(k_xcb_decide, dim3((unsigned)ceil_div(c, 64)), dim3(64), 0, s, rows, c, ignore_phase);
  hipLaunchKernelGGL(k_xcb_exact7, dim3(8, (unsigned)c), dim3(256), 0, s, a, a_pitch, na, b, b_pitch, nb, rows);
  hipLaunchKernelGGL(k_xcb_final, dim3((unsigned)ceil_div(c, 64)), dim3(64), 0, s, (const XcbRow*)rows, c, na, ignore_phase, delay, corr,
                     status);
}

// ---- X2 sectioned batch (k_xcs_*): rows longer than one transform, correlated by DIAGONALS of section pairs --------------
// Rows are cut into sections of S samples (P of a, Q of b; transforms of N = 2 S points).  Correlation is bilinear: the
// section pair (p, q) contributes its N-point correlation at the lag offset (p - q) S, so all pairs of one diagonal
// d = p - q share ONE spectrum C_d = sum_{p - q = d} A_p conj(B_q) and one transform back.  M = max(P, Q) transforms of
// z_s = a_s/|a| + i b_s/|b| and D = P + Q - 1 transforms of the C_d replace the 2 P Q of the pair-by-pair form; every row
// of a pass goes through the same launches.  Layout of a pass: Z[w][s][N], s < M (stride M N per row) for the section
// spectra, C[w][di][N], di = d + Q - 1 < D, for the diagonals and, after the second transform, their lags.
// z_s of every row: section s of both sides, zero-padded to N; a side that has run out of sections contributes zeros
__global__ __launch_bounds__(256) void k_xcs_pack(const double* __restrict__ a, int64_t a_pitch, int64_t na,
                                                  const double* __restrict__ b, int64_t b_pitch, int64_t nb,
                                                  const XcbRow* __restrict__ rows, float2* __restrict__ Z, int64_t S, int64_t M) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, s = blockIdx.y, w = blockIdx.z, N = 2 * S;
  if (i >= N) return;
  const int64_t t = s * S + i;
  float2 z = make_float2(0.0f, 0.0f);
  if (i < S) {
    if (t < na) z.x = (float)(a[w * a_pitch + t] / rows[w].norms[0]);
    if (t < nb) z.y = (float)(b[w * b_pitch + t] / rows[w].norms[1]);
  }
  Z[(w * M + s) * N + i] = z;
}
// conj(C_d) at bins k and N - k (k <= N/2) of diagonal di = d + Q - 1: A_p and B_q are untangled from Z_p, Z_q at the bin and
// its mirror like k_xcb_cross does, and the <= min(P, Q) products of the diagonal are summed in float64 in the order of p.
// One thread serves both bins of a mirror pair: the signals are real, so C_d[N-k] is the conjugate of C_d[k].
__global__ __launch_bounds__(256) void k_xcs_diag(const float2* __restrict__ Z, float2* __restrict__ C, int64_t N, int P, int Q) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x, w = blockIdx.z;
  if (k > N / 2) return;
  const int di = blockIdx.y, d = di - (Q - 1), M = P > Q ? P : Q, D = P + Q - 1;
  const int64_t km = (N - k) & (N - 1);
  const int p0 = d > 0 ? d : 0, p1 = d + Q - 1 < P - 1 ? d + Q - 1 : P - 1;
  const float2* Zw = Z + w * M * N;
  double cx = 0.0, cy = 0.0;
  for (int p = p0; p <= p1; ++p) {
    const float2* Zp = Zw + (int64_t)p * N;
    const float2* Zq = Zw + (int64_t)(p - d) * N;
    const float2 pk = Zp[k], pm = Zp[km], qk = Zq[k], qm = Zq[km];
    // A = (Zp[k] + conj Zp[N-k]) / 2, B = (Zq[k] - conj Zq[N-k]) / (2i); at bin N-k both are the conjugates (real signals)
    const float2 A = make_float2(0.5f * (pk.x + pm.x), 0.5f * (pk.y - pm.y));
    const float2 B = make_float2(0.5f * (qk.y + qm.y), -0.5f * (qk.x - qm.x));
    cx += (double)A.x * (double)B.x + (double)A.y * (double)B.y;           // A conj(B)
    cy += (double)A.y * (double)B.x - (double)A.x * (double)B.y;
  }
  float2* Cd = C + (w * D + di) * N;
  Cd[k] = make_float2((float)cx, (float)-cy);                              // the conjugate, for the forward-as-inverse transform
  if (km != k) Cd[km] = make_float2((float)cx, (float)cy);                 // C_d[N-k] = conj C_d[k]
}
// Lag j of row w's 'same' span out of the D transformed diagonals: l = j + (nb-1)//2 - (nb-1) is the lag in samples and
// full[l] = sum_d c_d[l - d S] over |l - d S| < S: at most two diagonals, d0 = floor(l / S) and d0 + 1, added in that order.
struct XcLagsOfSect {
  const float2* __restrict__ Y;                    // [rows][D][N], the second transform's output
  int64_t S;
  int P, Q;
  __device__ auto row(int64_t w, int64_t nb) const {
    const int D = P + Q - 1, q1 = Q - 1, ls = 63 - __builtin_clzll((unsigned long long)S);
    const int64_t n = 2 * S, s = S, off = (nb - 1) / 2 - (nb - 1);
    const float2* Yw = Y + w * D * n;
    const double dN = (double)n;
    return [=](int64_t j) {
      const int64_t l = j + off, d0 = l >> ls, m0 = l - d0 * s;             // floor division: m0 in [0, S)
      const int64_t i0 = d0 + q1, i1 = i0 + 1;
      double v = 0.0;
      if (i0 >= 0 && i0 < D) v = (double)Yw[i0 * n + m0].x / dN;
      if (m0 > 0 && i1 >= 0 && i1 < D) v += (double)Yw[i1 * n + (m0 + s)].x / dN;      // m0 - S, modulo N
      return v;
    };
  }
};
// same_out[w][j] = the doubles k_xcb_peak compares (grid: x over lags, y over rows)
__global__ __launch_bounds__(256) void k_xcs_same(XcLagsOfSect src, int64_t na, int64_t nb, double* __restrict__ same_out,
                                                  int64_t same_pitch) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x, w = blockIdx.y;
  if (j >= na) return;
  const auto lag = src.row(w, nb);
  same_out[w * same_pitch + j] = lag(j);
}
// norms[w] = (|a_w|, |b_w|) out of the row records
__global__ __launch_bounds__(64) void k_xcs_norms_out(const XcbRow* __restrict__ rows, int64_t count, double* __restrict__ norms) {
  const int64_t w = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (w >= count) return;
  norms[2 * w] = rows[w].norms[0];
  norms[2 * w + 1] = rows[w].norms[1];
}

// out[w][i] = (double)sig[(starts[w] + i - pad_l[w]) * stride] inside the window's samples, 0.0 in its padding
// (Spectrum.get_signal, util/spectrum.py:158-171, for a batch of windows; grid: x over samples, y over windows)
__global__ __launch_bounds__(256) void k_gather_windows(const float* __restrict__ sig, int64_t sig_stride, int64_t n,
                                                        const long long* __restrict__ starts, const long long* __restrict__ lens,
                                                        const long long* __restrict__ pad_l, int64_t w0, int64_t n_out,
                                                        double* __restrict__ out, int64_t out_pitch) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, w = w0 + blockIdx.y;
  if (i >= n_out) return;
  const long long k = i - pad_l[w], src = starts[w] + k;
  double v = 0.0;
  if (k >= 0 && k < lens[w] && src >= 0 && src < n) v = (double)sig[src * sig_stride];
  out[w * out_pitch + i] = v;
}

// ISTFT stage 1: frame f -> window * irfft(spec[f] * sqrt(n_fft))   (util/fourier.py:359, :401)
// irfft of H+1 bins via an H-point complex inverse FFT (conjugate trick on the forward core).
template <int LOGH>
__global__ __launch_bounds__(FftGeom<LOGH>::Threads) void k_istft_frames(const float2* __restrict__ spec, int64_t n_frames,
                                                                          const float* __restrict__ window,
                                                                          const float2* __restrict__ tw,
                                                                          const float2* __restrict__ post,
                                                                          float* __restrict__ frames, float scale) {
  using G = FftGeom<LOGH>;
  constexpr int H = G::H, T = G::T, bins = H + 1;
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  const int f = threadIdx.x / T, j = threadIdx.x - f * T;
  float2* X = lds + f * G::FrameLds;
  const int64_t fr = (int64_t)blockIdx.x * G::Frames + f;
  const bool live = fr < n_frames;
  // conj(Z[k]) with Z[k] = E[k] + i*O[k],  E = (X[k]+conj(X[H-k]))/2,  O = conj(W^k)*(X[k]-conj(X[H-k]))/2
  // (numpy's irfft ignores the imaginary parts of the DC and Nyquist bins.)
  float2 v[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int k = j + q * T;
    float2 z = make_float2(0.0f, 0.0f);
    if (live) {
      float2 a = spec[fr * bins + k];
      float2 b = spec[fr * bins + (H - k)];
      if (k == 0) {
        a.y = 0.0f;
        b.y = 0.0f;
      }
      b = cconj(b);
      const float2 ev = cadd(a, b);
      const float2 od = cmul(cconj(post[k]), csub(a, b));
      z = make_float2(0.5f * (ev.x - od.y), -0.5f * (ev.y + od.x));     // conj(0.5*(ev + i*od))
    }
    v[q] = z;
  }
  fft_core<LOGH>(v, X, j, tw);
  if (!live) return;
  // z_time[i] = conj(FFT(conj(Z)))[i] / H ; y[2i] = re, y[2i+1] = im
  for (int i = j; i < H; i += T) {
    const float2 r = X[lpad(i)];
    float2 o;
    o.x = r.x * scale * window[2 * i];
    o.y = -r.y * scale * window[2 * i + 1];
    reinterpret_cast<float2*>(frames)[fr * H + i] = o;
  }
}

// ISTFT of frames above 8192 points (r04): the irfft of one frame through the four-step complex transform K_stft uses for
// frames of that size (big_fft_c2c), `batch` frames at a time.
//   k_ibig_pack    A[b][k] = conj(Z[k]),  Z[k] = ((X[k] + conj X[H-k]) + i e^(i pi k / H) (X[k] - conj X[H-k])) / 2   (k < H)
//   big_fft_c2c    V = FFT_H(A);  z = conj(V) / H  is the packed frame: y[2 i] = Re z[i], y[2 i + 1] = Im z[i]
//   k_ibig_unpack  frames[f][n] = window[n] y[n] sqrt(n_fft)      (util/fourier.py:359, :401), then k_istft_ola as below
__global__ __launch_bounds__(256) void k_ibig_pack(const float2* __restrict__ spec, int64_t frame0, int64_t batch, int64_t H,
                                                   float2* __restrict__ A) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= batch * H) return;
  const int64_t b = t / H, k = t - b * H;
  const float2* X = spec + (frame0 + b) * (H + 1);
  float2 a = X[k], c = X[H - k];
  if (k == 0) {                                    // numpy's irfft ignores the imaginary parts of the DC and Nyquist bins
    a.y = 0.0f;
    c.y = 0.0f;
  }
  c = cconj(c);
  double sn, cs;
  sincospi((double)k / (double)H, &sn, &cs);       // e^(+i pi k / H)
  const float2 ev = cadd(a, c), df = csub(a, c);
  const float2 od = make_float2((float)(cs * df.x - sn * df.y), (float)(cs * df.y + sn * df.x));
  A[t] = make_float2(0.5f * (ev.x - od.y), -0.5f * (ev.y + od.x));          // conj((ev + i od) / 2)
}

__global__ __launch_bounds__(256) void k_ibig_unpack(const float2* __restrict__ V, int64_t frame0, int64_t batch, int64_t H,
                                                     const float* __restrict__ window, float* __restrict__ frames, float scale) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= batch * H) return;
  const int64_t b = t / H, i = t - b * H;
  const float2 r = V[t];
  reinterpret_cast<float2*>(frames)[(frame0 + b) * H + i] = make_float2(r.x * scale * window[2 * i], -r.y * scale * window[2 * i + 1]);
}

// ISTFT stage 2: gather-form overlap-add + window-sumsquare normalisation (no atomics):
// y[t] = sum_f frames[f][T - f*hop] / sum_f win^2[T - f*hop],  T = t + skip   (:405-416)
__global__ __launch_bounds__(256) void k_istft_ola(const float* __restrict__ frames, int64_t n_frames, int n_fft, int hop,
                                                    const float* __restrict__ window, float* __restrict__ y,
                                                    int64_t y_len, int64_t skip) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= y_len) return;
  const int64_t T = t + skip;
  const int64_t ola_len = (int64_t)n_fft + (int64_t)hop * (n_frames - 1);
  float acc = 0.0f, env = 0.0f;
  if (T < ola_len) {
    int64_t f_hi = T / hop;
    if (f_hi > n_frames - 1) f_hi = n_frames - 1;
    int64_t f_lo = (T - n_fft + hop) / hop;         // ceil((T - n_fft + 1)/hop)
    if (T - n_fft + 1 <= 0) f_lo = 0;
    for (int64_t f = f_lo; f <= f_hi; ++f) {
      const int64_t off = T - f * hop;
      if (off < 0 || off >= n_fft) continue;
      const float w = window[off];
      acc += frames[f * n_fft + off];
      env += w * w;
    }
    if (env > 1.17549435e-38f) acc /= env;          // > tiny(float32)  (:414-415)
  }
  y[t] = acc;
}

// Fused ISTFT: the [n_frames][n_fft] time-frame array never exists in HBM (at hop = n_fft/16 it is 16x the signal,
// written once and read once by the two-kernel path).  A workgroup owns NF = Frames*s consecutive frames,
// s = ceil(n_fft/hop) being the spacing at which frames stop overlapping.  Round r = 0..s-1 inverse-transforms the
// Frames frames F0 + r + u*s: they are pairwise disjoint in time, so each frame's own lanes add it straight into
// the LDS overlap-add accumulator with plain read-modify-writes; one workgroup barrier per round orders the
// rounds.  The summation order per sample is fixed (by round), so results are reproducible run to run.
// The workgroup writes the (NF - s + 1)*hop samples that only its own frames cover; the s-1 frames on either side
// are transformed by the neighbour as well ((s-1)/NF extra work: 12 % at 512/32).
__host__ __device__ constexpr bool istft_tables_in_lds(int logh) { return logh <= 9; }

template <int LOGH>
__global__ __launch_bounds__(FftGeom<LOGH>::Threads) __attribute__((amdgpu_waves_per_eu(LOGH <= 9 ? 3 : 1))) void k_istft_fused(const float2* __restrict__ spec, int64_t n_frames,
                                                                         int hop, int s, const float* __restrict__ window,
                                                                         const float2* __restrict__ tw,
                                                                         const float2* __restrict__ post,
                                                                         float* __restrict__ y, int64_t y_len, int64_t skip,
                                                                         float scale) {
  using G = FftGeom<LOGH>;
  constexpr int H = G::H, T = G::T, bins = H + 1, n_fft = 2 * H;
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  float* acc = reinterpret_cast<float*>(lds + G::Frames * G::FrameLds);
  const int tid = threadIdx.x;
  const int u = tid / T, j = tid - u * T;
  float2* X = lds + u * G::FrameLds;
  const int NF = G::Frames * s;
  const int out_frames = NF - s + 1;
  const int acc_len = (NF - 1) * hop + n_fft;
  const int64_t F0 = (int64_t)blockIdx.x * out_frames - (s - 1);      // first frame of the workgroup (may be < 0)
  for (int i = tid; i < acc_len; i += G::Threads) acc[i] = 0.0f;
  // window taps and untangle twiddles are the same for every frame: they live in LDS, not in 32 registers per lane
  // (n_fft <= 1024; the larger transforms keep their LDS for the overlap-add span and read the tables from memory)
  constexpr bool kTab = istft_tables_in_lds(LOGH);
  float* wl = acc + acc_len;                                           // [n_fft]
  float2* pl = reinterpret_cast<float2*>(wl + n_fft);                  // [H] conj(post)
  if (kTab) {
    for (int i = tid; i < n_fft; i += G::Threads) wl[i] = window[i];
    for (int i = tid; i < H; i += G::Threads) pl[i] = cconj(post[i]);
    __syncthreads();
  }
  // Occupancy hides the spectrum fetch: with the tables in LDS and no register double buffer the kernel fits 3 waves
  // per SIMD (146 VGPRs at n_fft = 512; the double-buffered form needed 216 = 2 waves and was 16 % slower, measured).
  float2 pa[8], pb[8], pk[8], wq[8];        // pk / wq: the tables in registers, large transforms only
  if (!kTab) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      pk[q] = cconj(post[j + q * T]);
      wq[q] = *reinterpret_cast<const float2*>(window + 2 * (j + q * T));
    }
  }
  // A frame outside [0, n_frames) is transformed like any other and dropped at the overlap-add (`live` below): its rows
  // only have to be readable, so the row index is clamped instead of selecting zeros element by element (32 v_cndmask per
  // round).  Whatever the clamped row holds -- NaNs included -- never reaches the accumulator.
  auto fetch = [&](int r) {
    if (r >= s) return;
    int64_t fr = F0 + r + u * s;
    fr = fr < 0 ? 0 : (fr >= n_frames ? n_frames - 1 : fr);
    const float2* row = spec + fr * bins;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int k = j + q * T;
      pa[q] = row[k];
      pb[q] = row[H - k];
    }
  };
  if (!kTab) fetch(0);                       // large transforms run at 2 waves per SIMD either way: keep their register
  for (int r = 0; r < s; ++r) {              // double buffer (round r+1 in flight under round r's butterflies)
    if (kTab) fetch(r);
    const int lf = r + u * s;                                         // frame index inside the workgroup
    const int64_t fr = F0 + lf;
    const bool live = fr >= 0 && fr < n_frames;
    float2 v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int k = j + q * T;
      float2 a = pa[q], b = pb[q];
      if (k == 0) {
        a.y = 0.0f;
        b.y = 0.0f;
      }
      b = cconj(b);
      const float2 ev = cadd(a, b);
      const float2 od = cmul(kTab ? pl[k] : pk[q], csub(a, b));
      v[q] = make_float2(0.5f * (ev.x - od.y), -0.5f * (ev.y + od.x));   // zeros stay zeros for a dead frame
    }
    if (!kTab) fetch(r + 1);
    fft_core<LOGH>(v, X, j, tw);
    __syncthreads();                                                  // the previous round's adds (and the zeroing) are done
    if (live) {
      float* dst = acc + lf * hop;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int i = j + q * T;
        const float2 z = X[lpad(i)];                                  // conj(FFT(conj Z)): y[2i] = re, y[2i+1] = -im
        const float2 wv = kTab ? *reinterpret_cast<const float2*>(wl + 2 * i) : wq[q];
        const float a0 = z.x * scale * wv.x, a1 = -z.y * scale * wv.y;
        if ((hop & 1) == 0) {
          float2 t = *reinterpret_cast<float2*>(dst + 2 * i);
          t.x += a0;
          t.y += a1;
          *reinterpret_cast<float2*>(dst + 2 * i) = t;
        } else {
          dst[2 * i] += a0;
          dst[2 * i + 1] += a1;
        }
      }
    }
  }
  __syncthreads();
  if (!kTab) {
    wl = reinterpret_cast<float*>(lds);                                // frame slots are free now: stage the window there
    for (int i = tid; i < n_fft; i += G::Threads) wl[i] = window[i];
    __syncthreads();
  }
  const int64_t ola_len = (int64_t)n_fft + (int64_t)hop * (n_frames - 1);
  const int out_len = out_frames * hop;
  const int64_t TT0 = (int64_t)blockIdx.x * out_len;                  // overlap-add coordinate of the first owned sample
  // Window-sumsquare envelope.  Away from the two ends of the signal every frame that can cover a sample exists, and the
  // envelope depends on the sample's phase TT mod hop alone: one table of hop sums per workgroup (same order of terms
  // as the general loop below: frames ascending = window offsets descending) replaces two 64-bit divisions and a
  // 16-term loop PER SAMPLE (they were a third of the kernel's instructions at 512/32).
  float* env_tab = wl + n_fft;          // kTab: behind the window (pl is dead now); else behind the staged window in the frame slots
  const bool use_tab = kTab || n_fft + hop <= 2 * G::Frames * G::FrameLds;
  // hop > n_fft leaves a gap of hop - n_fft samples behind every frame (phases >= n_fft) that no frame covers: the table has no
  // entry for them (it holds min(hop, n_fft) sums, which is what the LDS behind the window has room for) and the store loop
  // below writes their zero without touching the window, the table or the accumulator, whose last frame ends at its n_fft.
  const int tab_len = hop < n_fft ? hop : n_fft;
  if (use_tab) {
    for (int ph = tid; ph < tab_len; ph += G::Threads) {
      float env = 0.0f;
      for (int o = ph + ((n_fft - 1 - ph) / hop) * hop; o >= 0; o -= hop) env += wl[o] * wl[o];
      env_tab[ph] = env;
    }
    __syncthreads();
  }
  const int64_t interior_lo = n_fft - 1, interior_hi = (int64_t)hop * (n_frames - 1);     // all covering frames exist in [lo, hi]
  const int step_ph = G::Threads % hop;
  int ph = tid % hop;                                                  // TT0 is a multiple of hop: phase of TT = phase of p
  for (int p = tid; p < out_len; p += G::Threads, ph = ph + step_ph >= hop ? ph + step_ph - hop : ph + step_ph) {
    const int64_t TT = TT0 + p, t = TT - skip;
    if (t < 0) continue;
    if (t >= y_len) break;
    float a = 0.0f;
    if (TT < ola_len && ph < n_fft) {                                  // (ph >= n_fft: a gap sample, see the table above)
      float env;
      if (use_tab && TT >= interior_lo && TT <= interior_hi) {
        env = env_tab[ph];
      } else {
        int64_t e_hi = TT / hop;
        if (e_hi > n_frames - 1) e_hi = n_frames - 1;
        const int64_t e_lo = (TT - n_fft + 1 <= 0) ? 0 : (TT - n_fft + hop) / hop;
        env = 0.0f;
        for (int64_t e = e_lo; e <= e_hi; ++e) {
          const float w = wl[TT - e * hop];
          env += w * w;
        }
      }
      a = acc[p + (s - 1) * hop];
      if (env > 1.17549435e-38f) a /= env;                           // > tiny(float32)  (:414-415)
    }
    y[t] = a;
  }
}

// bytes of LDS the fused ISTFT needs for (n_fft, hop); it is used when they fit 64 KB
template <int LOGH>
static inline size_t istft_fused_lds(int hop) {
  using G = FftGeom<LOGH>;
  const int64_t n_fft = 2 * G::H, s = (n_fft + hop - 1) / hop;
  return G::FramesLds + (size_t)((G::Frames * s - 1) * hop + n_fft) * sizeof(float) +
         (istft_tables_in_lds(LOGH) ? (size_t)n_fft * sizeof(float) + (size_t)G::H * sizeof(float2) : 0);   // + the tables
}
static inline size_t istft_fused_lds_any(int n_fft, int hop) {
  size_t lds = (size_t)-1;
  if (n_fft >= 16 && (n_fft & (n_fft - 1)) == 0)
    (void)dispatch_logh<3, 12>(ilog2(n_fft / 2), [&](auto lh) {
      lds = istft_fused_lds<decltype(lh)::value>(hop);
      return PAR_OK;
    });
  return lds;
}
// Largest n_fft that takes the fused kernel.  A workgroup re-transforms s - 1 = n_fft/hop - 1 frames of its neighbour; with
// 8 or 4 frames side by side (n_fft <= 1024) that is 13-23 % extra work for never storing the frames, at 2048 (2 frames)
// the two forms are within 9 %, and a 4096-point frame fills the workgroup alone: s frames transformed per hop of
// output (tools/bench_istft_sweep.py, 23 M samples: 4096 at hop n/4, n/8, n/16 took 0.78 / 2.44 / 8.65 ms fused against
// 0.37 / 0.68 / 1.27 ms through the frame array).
#ifndef PAR_ISTFT_FUSE_MAX
#define PAR_ISTFT_FUSE_MAX 2048
#endif
static inline bool istft_is_fused(int n_fft, int hop) {
  return hop >= 1 && n_fft <= PAR_ISTFT_FUSE_MAX && istft_fused_lds_any(n_fft, hop) <= 64 * 1024;
}

// ---- renoiser gate (renoiser_gui.py:273-319, ABI 108) ------------------------------------------------------------------------
// get_mask_fac: a bin passes unchanged when float32(20 log10(float32(|X| + 1e-7))) > final[k], else it is multiplied by the
// float32 factor 10^(gain/20).  float32 20 log10 is monotone, so the host turns each threshold into one float32 magnitude
// cutoff c[k] (renoiser.gate_cutoffs): "passes" is then |X| + 1e-7 >= c[k] -- no transcendental per bin, and a NaN cutoff
// gates every bin.  |X| is the float32 value numpy's np.abs gives for complex64 (np_abs.h: correctly rounded division and
// square root; the native v_sqrt_f32 this function used before gated 12.8 % of the bins that sit exactly on their cutoff).
// Contraction off: the product and the + 1e-7 round separately, as numpy's do.
__device__ __forceinline__ float gate_mag(float re, float im) {
#pragma clang fp contract(off)
  const float mag = np_abs_c64(re, im);
  return mag + 1e-7f;
}
// X * fac as numpy multiplies complex64 by a float32 (fac becomes fac + 0i): the products with the zero imaginary part are kept
// -- they decide the signs of zero parts (and NaNs from infinite parts) exactly as numpy's do, a passing bin included
__device__ __forceinline__ float2 gate_bin(float2 v, float cut, float low) {
  const float f = gate_mag(v.x, v.y) >= cut ? 1.0f : low;
  return make_float2(v.x * f - v.y * 0.0f, v.x * 0.0f + v.y * f);
}

__global__ __launch_bounds__(256) void k_gate_spectrum(float2* __restrict__ spec, int64_t n_frames, int64_t bins, int64_t pitch,
                                                       const float* __restrict__ cutoff, float low) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= bins) return;
  const float cut = cutoff[b];
  for (int64_t f = blockIdx.y; f < n_frames; f += gridDim.y) {
    float2* p = spec + f * pitch + b;
    *p = gate_bin(*p, cut, low);
  }
}

// Fused gate: signal -> forward real FFT (K_stft mode 0's operations) -> gate -> irfft (K_istft's) -> window-sum-square
// overlap-add -> output, one launch, no spectrogram in HBM.  The signal is the reference's fix_length(x, n + n_fft/2): the
// appended zeros and the reflect boundary of that padded length are folded into the gather (no padded copy).
// Streaming form: a workgroup owns a run of NF = Frames * rounds consecutive frames and walks it Frames at a time.  Each
// round's frames go forward, through the gate (in registers: a lane holds the bin pairs (k, H - k) after the untangle), back
// (one LDS exchange forms the inverse input) and into an LDS ring of R floats; the ring positions every covering frame has
// reached are normalised, stored and cleared.  Only the first s - 1 frames of a run (s = ceil(n_fft / hop)) are also
// transformed by the neighbouring run.  Every sample sums its frames in ascending order.
template <int LOGH>
struct GateGeom {
  using G = FftGeom<LOGH>;
  static int rounds(int s) { return (int)ceil_div(12 * (int64_t)s, G::Frames); }          // (s - 1) / NF < 1/12 redundant
  static int ring(int hop) {
    int r = 1;
    while (r < 2 * G::H + G::Frames * hop) r <<= 1;
    return r;
  }
  static size_t lds(int hop) {
    return G::FramesLds + (size_t)(ring(hop) + hop) * sizeof(float);
  }
  // Waves per SIMD the register allocation must keep (the second __launch_bounds__ argument).  The 2048- and 8192-point kernels
  // sit at 168 VGPRs, the last count at which three waves fit; the correctly rounded square root of gate_mag took them to 169 and
  // 171, two waves, and 2048/512 from 1.31 to 1.69 ms.  The other sizes state what they had.
  static constexpr int kWaves = LOGH == 3 ? 7 : (LOGH == 11 ? 2 : 3);
};

template <int LOGH>
__global__ __launch_bounds__(FftGeom<LOGH>::Threads, GateGeom<LOGH>::kWaves) void k_gate_stft(const float* __restrict__ x, int64_t n,
                                                                      int64_t x_stride, int hop, int s, int rounds, int ring,
                                                                      const float* __restrict__ window, const float2* __restrict__ tw,
                                                                      const float2* __restrict__ post, const float* __restrict__ cutoff,
                                                                      float low, float* __restrict__ y, int64_t y_stride,
                                                                      int64_t n_frames_i, float fscale, float iscale) {
  using G = FftGeom<LOGH>;
  constexpr int H = G::H, T = G::T, n_fft = 2 * H, P = (H / 2) / T;
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  float* acc = reinterpret_cast<float*>(lds + G::Frames * G::FrameLds);
  float* env_tab = acc + ring;
  const int tid = threadIdx.x;
  const int u = tid / T, j = tid - u * T;
  float2* X = lds + u * G::FrameLds;
  x += blockIdx.y;                                   // channel
  y += blockIdx.y;
  const int64_t N = n + H;                           // fix_length(x, n + n_fft // 2)
  const int NF = G::Frames * rounds, OUT = NF - (s - 1);
  const int64_t TT_lo = (int64_t)blockIdx.x * OUT * hop, TT_hi = TT_lo + (int64_t)OUT * hop;   // owned overlap-add range
  const int64_t st_lo = TT_lo > H ? TT_lo : H, st_hi = TT_hi < N ? TT_hi : N;            // ... that is output: t = TT - H < n
  const int64_t f_start = (int64_t)blockIdx.x * OUT - (s - 1);
  const int64_t ola_len = (int64_t)n_fft + (int64_t)hop * (n_frames_i - 1);
  for (int i = tid; i < ring; i += G::Threads) acc[i] = 0.0f;
  // window-sum-square by phase where every covering frame exists (frames ascending = offsets descending, as K_istft)
  for (int ph = tid; ph < hop; ph += G::Threads) {
    float e = 0.0f;
    for (int o = ph + ((n_fft - 1 - ph) / hop) * hop; o >= 0; o -= hop) e += window[o] * window[o];
    env_tab[ph] = e;
  }
  // per-lane constants of every frame: window taps of the lane's points, untangle twiddles, the cutoffs of its bins
  float2 wq[8], pk[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    wq[q] = *reinterpret_cast<const float2*>(window + 2 * (j + q * T));
    pk[q] = cconj(post[j + q * T]);
  }
  float2 pw[P + 1];
  float ck[P + 1], cm[P];
#pragma unroll
  for (int i = 0; i < P; ++i) {
    pw[i] = post[j + i * T];
    ck[i] = cutoff[j + i * T];
    cm[i] = cutoff[H - j - i * T];
  }
  pw[P] = post[H / 2];
  ck[P] = cutoff[H / 2];
  const float hs = 0.5f * fscale;
  // inverse input z[k] = conj(0.5 (ev + i od)) of the gated bins a = X[k], b = X[H - k] (K_istft's operations)
  auto inv = [&](float2 a, float2 b, float2 cp, bool dc) {
    if (dc) {
      a.y = 0.0f;
      b.y = 0.0f;
    }
    b = cconj(b);
    const float2 ev = cadd(a, b);
    const float2 od = cmul(cp, csub(a, b));
    return make_float2(0.5f * (ev.x - od.y), -0.5f * (ev.y + od.x));
  };
  __syncthreads();
  const int64_t interior_lo = n_fft - 1, interior_hi = (int64_t)hop * (n_frames_i - 1);
  for (int r = 0; r < rounds; ++r) {
    const int64_t f0 = f_start + (int64_t)r * G::Frames;
    if (f0 * hop >= st_hi) break;                                   // workgroup-uniform: nothing left to store
    const int64_t fr = f0 + u;
    const bool live = fr >= 0 && fr < n_frames_i;
    // gather + window + pack (K_stft's products: window * sample)
    float2 v[8];
    const long long base = (long long)fr * hop - H;
    if (live && base >= 0 && base + n_fft <= n) {
      const float* xs = x + base * x_stride;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int t0 = 2 * (j + q * T);
        v[q] = make_float2(wq[q].x * xs[(int64_t)t0 * x_stride], wq[q].y * xs[(int64_t)(t0 + 1) * x_stride]);
      }
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int t0 = 2 * (j + q * T);
        float2 z = make_float2(0.0f, 0.0f);
        if (live) {
          const long long i0 = reflect_index(base + t0, N), i1 = reflect_index(base + t0 + 1, N);
          z.x = wq[q].x * (i0 < n ? x[i0 * x_stride] : 0.0f);
          z.y = wq[q].y * (i1 < n ? x[i1 * x_stride] : 0.0f);
        }
        v[q] = z;
      }
    }
    fft_core<LOGH>(v, X, j, tw);
    // untangle (K_stft mode 0: X[k] = (ev - i t) / 2 / sqrt(n_fft)), gate, and the inverse input of the same pair, written
    // back to the two slots this lane just read (the pair sets of the lanes are disjoint)
#pragma unroll
    for (int i = 0; i <= P; ++i) {
      const int k = (i < P) ? j + i * T : H / 2;
      if (i == P && j != 0) break;
      const int sk = lpad(k), sm = lpad((H - k) & (H - 1));
      const float2 zk = X[sk];
      const float2 zc = cconj(X[sm]);
      const float2 ev = cadd(zk, zc);
      const float2 t = cmul(pw[i], csub(zk, zc));
      const float2 gk = gate_bin(make_float2((ev.x + t.y) * hs, (ev.y - t.x) * hs), ck[i], low);
      if (i == P) {                                                  // k = H/2 pairs with itself
        X[sk] = inv(gk, gk, cconj(post[H / 2]), false);
      } else {
        const float2 gm = gate_bin(make_float2((ev.x - t.y) * hs, (-ev.y - t.x) * hs), cm[i], low);   // bin H - k
        X[sk] = inv(gk, gm, pk[i], k == 0);
        if (k != 0) X[sm] = inv(gm, gk, cconj(post[H - k]), false);
      }
    }
    frame_sync<T>();
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = X[lpad(j + q * T)];
    fft_core<LOGH>(v, X, j, tw);
    // windowed time samples, in place: y[2i] = re, y[2i+1] = -im of conj(FFT(conj Z)) (K_istft's scaling)
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int i = j + q * T;
      const float2 z = X[lpad(i)];
      X[lpad(i)] = make_float2(z.x * iscale * wq[q].x, -z.y * iscale * wq[q].y);
    }
    __syncthreads();
    // overlap-add of the round's frames into the ring, frames ascending
    const int span = (G::Frames - 1) * hop + n_fft;
    for (int p = tid; p < span; p += G::Threads) {
      int u_hi = p / hop;
      if (u_hi > G::Frames - 1) u_hi = G::Frames - 1;
      const int u_lo = p - n_fft + 1 <= 0 ? 0 : (p - n_fft + hop) / hop;
      float* slot = acc + ((f0 * hop + p) & (ring - 1));
      float a = *slot;
      for (int w = u_lo; w <= u_hi; ++w) {
        const int64_t fw = f0 + w;
        if (fw < 0 || fw >= n_frames_i) continue;
        const int off = p - w * hop;
        const float2 pr = lds[w * G::FrameLds + lpad(off >> 1)];
        a += (off & 1) ? pr.y : pr.x;
      }
      *slot = a;
    }
    __syncthreads();
    // the round completes [f0 hop, (f0 + Frames) hop): normalise and store what this run owns, clear the ring slots
    for (int p = tid; p < G::Frames * hop; p += G::Threads) {
      const int64_t TT = f0 * hop + p;
      float* slot = acc + (TT & (ring - 1));
      float a = *slot;
      *slot = 0.0f;
      if (TT < TT_lo || TT < st_lo || TT >= st_hi) continue;
      if (TT < ola_len) {
        float env;
        if (TT >= interior_lo && TT <= interior_hi) {
          env = env_tab[TT % hop];
        } else {
          int64_t e_hi = TT / hop;
          if (e_hi > n_frames_i - 1) e_hi = n_frames_i - 1;
          const int64_t e_lo = (TT - n_fft + 1 <= 0) ? 0 : (TT - n_fft + hop) / hop;
          env = 0.0f;
          for (int64_t e = e_lo; e <= e_hi; ++e) {
            const float w = window[TT - e * hop];
            env += w * w;
          }
        }
        if (env > 1.17549435e-38f) a /= env;                          // > tiny(float32)  (util/fourier.py:414-415)
      } else {
        a = 0.0f;
      }
      y[(TT - H) * y_stride] = a;
    }
  }
}

// ---- MaxMono dropout repair (dropouts_gui.py:137-163, added at ABI 109) ------------------------------------------------------------
// D_max = where(|D_L| > |D_R|, D_L, D_R), D_min = where(|D_L| < |D_R|, D_L, D_R): a tie and a NaN magnitude give D_R in both.
// The magnitudes are numpy's complex64 np.abs (np_abs.h); the selection copies the chosen bin's bits, it multiplies nothing.
__device__ __forceinline__ void select_bin(float2 l, float2 r, float2& mx, float2& mn) {
  const float ml = np_abs_c64(l.x, l.y), mr = np_abs_c64(r.x, r.y);
  mx = ml > mr ? l : r;
  mn = ml < mr ? l : r;
}

__global__ __launch_bounds__(256) void k_select_spectrum(const float2* __restrict__ specL, const float2* __restrict__ specR,
                                                         int64_t n_frames, int64_t bins, int64_t pitch, float2* __restrict__ out_max,
                                                         float2* __restrict__ out_min) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= bins) return;
  for (int64_t f = blockIdx.y; f < n_frames; f += gridDim.y) {
    float2 mx, mn;
    select_bin(specL[f * pitch + b], specR[f * pitch + b], mx, mn);
    if (out_max) out_max[f * pitch + b] = mx;
    if (out_min) out_min[f * pitch + b] = mn;
  }
}

// Fused MaxMono: the two-channel, two-output sibling of k_gate_stft, with its runs, rounds and fix_length / reflect gather.
// Order of a round over ONE frame buffer: L forward -> the lane keeps L's bin pairs (k, H - k) in registers -> R forward ->
// select in registers -> the inverse input of the max spectrum goes to the frame, that of the min spectrum stays in registers
// -> max inverse, overlap-add into ring 0 -> min inverse input to the frame -> min inverse, overlap-add into ring 1 -> both
// rings' completed positions are normalised, stored and cleared.  The rings are exactly 2H + Frames * hop floats (not rounded
// to a power of two: at 8192 points two rounded rings alone would be 128 KB): a position's slot is its distance from the
// run's first sample modulo the ring, kept as one running base per round and a conditional subtract per position.
template <int LOGH>
struct MaxMonoGeom {
  using G = FftGeom<LOGH>;
  static int rounds(int s) { return GateGeom<LOGH>::rounds(s); }
  static int ring(int hop) { return 2 * G::H + G::Frames * hop; }
  static size_t lds(int hop) { return G::FramesLds + (size_t)(2 * ring(hop) + hop) * sizeof(float); }
  // Waves per SIMD the register allocation must keep: two at every size (K_maxmono, has the figures).  The second
  // channel's bin pairs and the second inverse input do not fit the 168 VGPRs of three waves: asked for three, every size from
  // 32 points up spilled 128-372 bytes per lane and ran slower (10-min stereo: 2048/512 1.69 against 1.60 ms, 2048/128 5.83
  // against 5.50, 512/64 2.00 against 1.95; profiles/maxmono_waves_ab.json).  From 4096 points on the two rings leave LDS for two
  // waves anyway.  The figures hold with this file's -fno-slp-vectorize (build.py): without it the two largest sizes spill.
  static constexpr int kWaves = 2;
};

template <int LOGH>
__global__ __launch_bounds__(FftGeom<LOGH>::Threads, MaxMonoGeom<LOGH>::kWaves) void k_maxmono_stft(
    const float* __restrict__ xL, const float* __restrict__ xR, int64_t n, int64_t x_stride, int hop, int s, int rounds, int ring,
    const float* __restrict__ window, const float2* __restrict__ tw, const float2* __restrict__ post, float* __restrict__ y_max,
    int64_t ymax_stride, float* __restrict__ y_min, int64_t ymin_stride, int64_t n_frames_i, float fscale, float iscale) {
  using G = FftGeom<LOGH>;
  constexpr int H = G::H, T = G::T, n_fft = 2 * H, P = (H / 2) / T;
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  float* acc_max = reinterpret_cast<float*>(lds + G::Frames * G::FrameLds);
  float* acc_min = acc_max + ring;
  float* env_tab = acc_min + ring;
  const int tid = threadIdx.x;
  const int u = tid / T, j = tid - u * T;
  float2* X = lds + u * G::FrameLds;
  const int64_t N = n + H;                           // fix_length(x, n + n_fft // 2)
  const int NF = G::Frames * rounds, OUT = NF - (s - 1);
  const int64_t TT_lo = (int64_t)blockIdx.x * OUT * hop, TT_hi = TT_lo + (int64_t)OUT * hop;   // owned overlap-add range
  const int64_t st_lo = TT_lo > H ? TT_lo : H, st_hi = TT_hi < N ? TT_hi : N;            // ... that is output: t = TT - H < n
  const int64_t f_start = (int64_t)blockIdx.x * OUT - (s - 1);
  const int64_t ola_len = (int64_t)n_fft + (int64_t)hop * (n_frames_i - 1);
  for (int i = tid; i < 2 * ring; i += G::Threads) acc_max[i] = 0.0f;
  // window-sum-square by phase where every covering frame exists (frames ascending = offsets descending, as K_istft)
  for (int ph = tid; ph < hop; ph += G::Threads) {
    float e = 0.0f;
    for (int o = ph + ((n_fft - 1 - ph) / hop) * hop; o >= 0; o -= hop) e += window[o] * window[o];
    env_tab[ph] = e;
  }
  // per-lane constants of every frame: window taps of the lane's points, untangle twiddles
  float2 wq[8], pk[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    wq[q] = *reinterpret_cast<const float2*>(window + 2 * (j + q * T));
    pk[q] = cconj(post[j + q * T]);
  }
  float2 pw[P + 1];
#pragma unroll
  for (int i = 0; i < P; ++i) pw[i] = post[j + i * T];
  pw[P] = post[H / 2];
  const float hs = 0.5f * fscale;
  // inverse input z[k] = conj(0.5 (ev + i od)) of the selected bins a = X[k], b = X[H - k] (K_istft's operations)
  auto inv = [&](float2 a, float2 b, float2 cp, bool dc) {
    if (dc) {
      a.y = 0.0f;
      b.y = 0.0f;
    }
    b = cconj(b);
    const float2 ev = cadd(a, b);
    const float2 od = cmul(cp, csub(a, b));
    return make_float2(0.5f * (ev.x - od.y), -0.5f * (ev.y + od.x));
  };
  __syncthreads();
  const int64_t interior_lo = n_fft - 1, interior_hi = (int64_t)hop * (n_frames_i - 1);
  int ring_base = 0;                                                  // slot of position f0 * hop
  for (int r = 0; r < rounds; ++r) {
    const int64_t f0 = f_start + (int64_t)r * G::Frames;
    if (f0 * hop >= st_hi) break;                                   // workgroup-uniform: nothing left to store
    const int64_t fr = f0 + u;
    const bool live = fr >= 0 && fr < n_frames_i;
    const long long base = (long long)fr * hop - H;
    // gather + window + pack (K_stft's products: window * sample) and the forward transform of one channel
    auto forward = [&](const float* __restrict__ x) {
      float2 v[8];
      if (live && base >= 0 && base + n_fft <= n) {
        const float* xs = x + base * x_stride;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int t0 = 2 * (j + q * T);
          v[q] = make_float2(wq[q].x * xs[(int64_t)t0 * x_stride], wq[q].y * xs[(int64_t)(t0 + 1) * x_stride]);
        }
      } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int t0 = 2 * (j + q * T);
          float2 z = make_float2(0.0f, 0.0f);
          if (live) {
            const long long i0 = reflect_index(base + t0, N), i1 = reflect_index(base + t0 + 1, N);
            z.x = wq[q].x * (i0 < n ? x[i0 * x_stride] : 0.0f);
            z.y = wq[q].y * (i1 < n ? x[i1 * x_stride] : 0.0f);
          }
          v[q] = z;
        }
      }
      fft_core<LOGH>(v, X, j, tw);
    };
    // untangle (K_stft mode 0: X[k] = (ev - i t) / 2 / sqrt(n_fft)) of the pair i: bins k and H - k
    auto untangle = [&](int i, int sk, int sm, float2& bk, float2& bm) {
      const float2 zk = X[sk];
      const float2 zc = cconj(X[sm]);
      const float2 ev = cadd(zk, zc);
      const float2 t = cmul(pw[i], csub(zk, zc));
      bk = make_float2((ev.x + t.y) * hs, (ev.y - t.x) * hs);
      bm = make_float2((ev.x - t.y) * hs, (-ev.y - t.x) * hs);
    };
    forward(xL);
    float2 lk[P + 1], lm[P + 1];
#pragma unroll
    for (int i = 0; i <= P; ++i) {
      const int k = (i < P) ? j + i * T : H / 2;
      if (i == P && j != 0) break;
      untangle(i, lpad(k), lpad((H - k) & (H - 1)), lk[i], lm[i]);
    }
    forward(xR);                                                     // its first exchange waits for the reads above
    // select, and the inverse inputs of the same pair: the max spectrum's written back to the two slots this lane just read
    // (the pair sets of the lanes are disjoint), the min spectrum's kept for the second inverse
    float2 zk_min[P + 1], zm_min[P + 1];
#pragma unroll
    for (int i = 0; i <= P; ++i) {
      const int k = (i < P) ? j + i * T : H / 2;
      if (i == P && j != 0) break;
      const int sk = lpad(k), sm = lpad((H - k) & (H - 1));
      float2 rk, rm, xk, nk, xm, nm;
      untangle(i, sk, sm, rk, rm);
      select_bin(lk[i], rk, xk, nk);
      if (i == P) {                                                  // k = H/2 pairs with itself
        const float2 cp = cconj(post[H / 2]);
        if (y_max) X[sk] = inv(xk, xk, cp, false);
        if (y_min) zk_min[i] = inv(nk, nk, cp, false);
      } else {
        select_bin(lm[i], rm, xm, nm);                               // bin H - k
        const float2 cpm = cconj(post[H - k]);
        if (y_max) {
          X[sk] = inv(xk, xm, pk[i], k == 0);
          if (k != 0) X[sm] = inv(xm, xk, cpm, false);
        }
        if (y_min) {
          zk_min[i] = inv(nk, nm, pk[i], k == 0);
          if (k != 0) zm_min[i] = inv(nm, nk, cpm, false);
        }
      }
    }
    // inverse transform of the frame buffer's inverse input, windowed, overlap-added into `acc`, frames ascending
    auto inverse_ola = [&](float* __restrict__ acc) {
      frame_sync<T>();
      float2 v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = X[lpad(j + q * T)];
      fft_core<LOGH>(v, X, j, tw);
      // windowed time samples, in place: y[2i] = re, y[2i+1] = -im of conj(FFT(conj Z)) (K_istft's scaling)
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int i = j + q * T;
        const float2 z = X[lpad(i)];
        X[lpad(i)] = make_float2(z.x * iscale * wq[q].x, -z.y * iscale * wq[q].y);
      }
      __syncthreads();
      const int span = (G::Frames - 1) * hop + n_fft;
      for (int p = tid; p < span; p += G::Threads) {
        int u_hi = p / hop;
        if (u_hi > G::Frames - 1) u_hi = G::Frames - 1;
        const int u_lo = p - n_fft + 1 <= 0 ? 0 : (p - n_fft + hop) / hop;
        int sl = ring_base + p;                                      // p < span <= ring
        if (sl >= ring) sl -= ring;
        float a = acc[sl];
        for (int w = u_lo; w <= u_hi; ++w) {
          const int64_t fw = f0 + w;
          if (fw < 0 || fw >= n_frames_i) continue;
          const int off = p - w * hop;
          const float2 pr = lds[w * G::FrameLds + lpad(off >> 1)];
          a += (off & 1) ? pr.y : pr.x;
        }
        acc[sl] = a;
      }
      __syncthreads();
    };
    if (y_max) inverse_ola(acc_max);
    if (y_min) {                                                     // a NULL output costs neither its inverse input nor its inverse
#pragma unroll
      for (int i = 0; i <= P; ++i) {
        const int k = (i < P) ? j + i * T : H / 2;
        if (i == P && j != 0) break;
        X[lpad(k)] = zk_min[i];
        if (i < P && k != 0) X[lpad(H - k)] = zm_min[i];
      }
      inverse_ola(acc_min);
    }
    // the round completes [f0 hop, (f0 + Frames) hop): normalise and store what this run owns, clear the ring slots
    for (int p = tid; p < G::Frames * hop; p += G::Threads) {
      const int64_t TT = f0 * hop + p;
      int sl = ring_base + p;
      if (sl >= ring) sl -= ring;
      float a = acc_max[sl], b = acc_min[sl];
      acc_max[sl] = 0.0f;
      acc_min[sl] = 0.0f;
      if (TT < TT_lo || TT < st_lo || TT >= st_hi) continue;
      if (TT < ola_len) {
        float env;
        if (TT >= interior_lo && TT <= interior_hi) {
          env = env_tab[TT % hop];
        } else {
          int64_t e_hi = TT / hop;
          if (e_hi > n_frames_i - 1) e_hi = n_frames_i - 1;
          const int64_t e_lo = (TT - n_fft + 1 <= 0) ? 0 : (TT - n_fft + hop) / hop;
          env = 0.0f;
          for (int64_t e = e_lo; e <= e_hi; ++e) {
            const float w = window[TT - e * hop];
            env += w * w;
          }
        }
        if (env > 1.17549435e-38f) {                                  // > tiny(float32)  (util/fourier.py:414-415)
          a /= env;
          b /= env;
        }
      } else {
        a = 0.0f;
        b = 0.0f;
      }
      if (y_max) y_max[(TT - H) * ymax_stride] = a;
      if (y_min) y_min[(TT - H) * ymin_stride] = b;
    }
    ring_base += G::Frames * hop;                                    // Frames * hop < ring
    if (ring_base >= ring) ring_base -= ring;
  }
}

}  // namespace par

extern "C" {

// frames per four-step batch of the big ISTFT: two complex arrays of batch x H points beside the frame array
static int64_t istft_big_batch(int64_t n_frames, int n_fft) {
  const int64_t H = n_fft / 2, want = (1ll << 22) / H;
  const int64_t b = want < 1 ? 1 : want;
  return b < n_frames ? b : n_frames;
}

int64_t par_istft_scratch_floats(int64_t n_frames, int n_fft, int hop) {
  if (n_frames < 1 || n_fft < 1 || hop < 1) return 0;
  if (n_fft > 8192) return n_frames * (int64_t)n_fft + 4 * istft_big_batch(n_frames, n_fft) * (int64_t)(n_fft / 2) + 16;
  return par::istft_is_fused(n_fft, hop) ? 0 : n_frames * (int64_t)n_fft;
}

int64_t par_stft_frames(int64_t n, int n_fft, int hop) {
  if (n < 1 || n_fft < 1 || hop < 1) return 0;
  return (n + 2 * (int64_t)(n_fft / 2) - n_fft) / hop + 1;
}

// The register path's transform sizes: M = n_fft * zeropad a power of two in [16, 16384] of an even n_fft
static bool stft_size_supported(int n_fft, int zeropad) {
  const int64_t M = (int64_t)n_fft * zeropad;
  return n_fft >= 2 && zeropad >= 1 && (n_fft % 2) == 0 && M >= 16 && M <= 16384 && (M & (M - 1)) == 0;
}
static int require_stft_size(const char* who, int n_fft, int zeropad) {
  PAR_REQUIRE(stft_size_supported(n_fft, zeropad), PAR_ERR_UNSUPPORTED, "%s: n_fft*zeropad=%lld is not a power of two in [16, 16384]", who,
              (long long)n_fft * zeropad);
  return PAR_OK;
}

int par_stft_f32(int device, const float* x, int64_t n, int64_t x_stride, int n_fft, int hop, int zeropad,
                 const float* window, float* out, int mode, int64_t out_pitch, void* stream) {
  using namespace par;
  PAR_REQUIRE(x && window && out, PAR_ERR_ARG, "par_stft_f32: null pointer");
  const int64_t pitch = out_pitch ? out_pitch : (int64_t)n_fft * zeropad / 2 + 1;     // elements (float or float2) between rows
  PAR_REQUIRE(pitch >= (int64_t)n_fft * zeropad / 2 + 1, PAR_ERR_ARG, "par_stft_f32: out_pitch %lld < bins", (long long)out_pitch);
  PAR_REQUIRE(n >= 1 && x_stride >= 1 && hop >= 1 && zeropad >= 1 && n_fft >= 2, PAR_ERR_ARG, "par_stft_f32: bad sizes");
  PAR_REQUIRE(mode == 0 || mode == 1, PAR_ERR_ARG, "par_stft_f32: mode must be 0 (complex) or 1 (magnitude)");
  int rc = require_stft_size("par_stft_f32", n_fft, zeropad);
  if (rc != PAR_OK) return rc;
  const int M = n_fft * zeropad, H = M / 2;
  PAR_HIP_CHECK(hipSetDevice(device));
  Twiddles tw;
  rc = get_twiddles(device, M, &tw);
  if (rc != PAR_OK) return rc;
  const int64_t n_frames = par_stft_frames(n, n_fft, hop);
  const float scale = (float)(1.0 / sqrt((double)n_fft));
  // (16384 points -- the GUI's 4096 x zero-padding 4 -- are one 1024-lane workgroup per frame and 72 KB of the CU's 160 KB of
  // LDS, above the 64 KB a kernel gets by default: raised per kernel once, here and in the fused consumers below)
  return dispatch_logh<3, 13>(ilog2(H), [&](auto lh) {
    return dispatch_bool(mode == 1, [&](auto mag) {
      return dispatch_bool(x_stride == 1, [&](auto unit) {
        using G = FftGeom<decltype(lh)::value>;
        return launch_with_lds(k_stft<decltype(lh)::value, decltype(mag)::value ? 1 : 0, decltype(unit)::value>, dim3(G::grid(n_frames)),
                               dim3(G::Threads), G::FramesLds, device, as_stream(stream), x, n, x_stride, n_fft, hop, window, tw.w, tw.post,
                               out, n_frames, scale, pitch);
      });
    });
  });
}

// Band dB straight out of the register-path transform (k_stft mode 2): out[f] = mean over b in [bin_l, bin_u) of
// 20 log10(|X_f[b]| / sqrt(n_fft) + 1e-7), float64, one value per frame of par_stft_frames(n, n_fft, hop).
int par_stft_band_db_f32(int device, const float* x, int64_t n, int64_t x_stride, int n_fft, int hop, int zeropad,
                         const float* window, int bin_l, int bin_u, double* out, void* stream) {
  using namespace par;
  PAR_REQUIRE(x && window && out, PAR_ERR_ARG, "par_stft_band_db_f32: null pointer");
  PAR_REQUIRE(n >= 1 && x_stride >= 1 && hop >= 1 && zeropad >= 1 && n_fft >= 2, PAR_ERR_ARG, "par_stft_band_db_f32: bad sizes");
  const int64_t M64 = (int64_t)n_fft * zeropad;
  PAR_REQUIRE(0 <= bin_l && bin_l < bin_u && (int64_t)bin_u <= M64 / 2 + 1, PAR_ERR_ARG,
              "par_stft_band_db_f32: empty or out-of-range band [%d, %d) of %lld bins", bin_l, bin_u, (long long)(M64 / 2 + 1));
  int rc = require_stft_size("par_stft_band_db_f32", n_fft, zeropad);
  if (rc != PAR_OK) return rc;
  const int M = (int)M64, H = M / 2;
  PAR_HIP_CHECK(hipSetDevice(device));
  Twiddles tw;
  rc = get_twiddles(device, M, &tw);
  if (rc != PAR_OK) return rc;
  const int64_t n_frames = par_stft_frames(n, n_fft, hop);
  const float scale = (float)(1.0 / sqrt((double)n_fft));
  const int64_t band = (int64_t)bin_l | ((int64_t)bin_u << 32);
  float* outf = reinterpret_cast<float*>(out);
  return dispatch_logh<3, 13>(ilog2(H), [&](auto lh) {
    return dispatch_bool(x_stride == 1, [&](auto unit) {
      using G = FftGeom<decltype(lh)::value>;
      // beside the frames: the waves' partial sums (frame_lane_sum)
      return launch_with_lds(k_stft<decltype(lh)::value, 2, decltype(unit)::value>, dim3(G::grid(n_frames)), dim3(G::Threads),
                             G::FramesLds + (size_t)G::Threads / kWave * sizeof(double), device, as_stream(stream), x, n, x_stride, n_fft,
                             hop, window, tw.w, tw.post, outf, n_frames, scale, band);
    });
  });
}

// Stereo balance boxes straight from the two channels (k_stft_pan): fac[b], count[b] as par_pan_ratio_f32 gives them on the
// mode-1 spectrograms of xL and xR, without the spectrograms.
size_t par_stft_pan_scratch_bytes(const int32_t* boxes_host, int64_t n_box) { return par::pan_scratch_bytes(boxes_host, n_box); }

int par_stft_pan_ratio_f32(int device, const float* xL, const float* xR, int64_t x_stride, int64_t n, int n_fft, int hop, int zeropad,
                           const float* window, const int32_t* boxes, const int32_t* boxes_host, int64_t n_box, double* fac,
                           int64_t* count, void* scratch, size_t scratch_bytes, void* stream) {
  using namespace par;
  PAR_REQUIRE(xL && xR && window && boxes && boxes_host && fac && count && scratch, PAR_ERR_ARG, "par_stft_pan_ratio_f32: null pointer");
  PAR_REQUIRE(n >= 1 && x_stride >= 1 && hop >= 1 && zeropad >= 1 && n_fft >= 2 && n_box >= 1 && n_box <= kPanMaxBoxes, PAR_ERR_ARG,
              "par_stft_pan_ratio_f32: bad sizes");
  PAR_REQUIRE(((uintptr_t)scratch & 15) == 0, PAR_ERR_ARG, "par_stft_pan_ratio_f32: scratch is not 16-byte aligned");
  int rc = require_stft_size("par_stft_pan_ratio_f32", n_fft, zeropad);
  if (rc != PAR_OK) return rc;
  const int M = n_fft * zeropad, H = M / 2;
  const int64_t n_frames = par_stft_frames(n, n_fft, hop);
  int64_t n_items = 0;
  rc = pan_check_boxes("par_stft_pan_ratio_f32", boxes_host, n_box, H + 1, n_frames, &n_items);
  if (rc != PAR_OK) return rc;
  PAR_REQUIRE(scratch_bytes >= pan_scratch_bytes(boxes_host, n_box), PAR_ERR_WORKSPACE, "par_stft_pan_ratio_f32: scratch %zu < %zu",
              scratch_bytes, pan_scratch_bytes(boxes_host, n_box));
  PAR_HIP_CHECK(hipSetDevice(device));
  Twiddles tw;
  rc = get_twiddles(device, M, &tw);
  if (rc != PAR_OK) return rc;
  hipStream_t s = as_stream(stream);
  const float scale = (float)(1.0 / sqrt((double)n_fft));
  const int64_t* offs = reinterpret_cast<const int64_t*>(scratch);
  PanPart* part = reinterpret_cast<PanPart*>(reinterpret_cast<char*>(scratch) + pan_offs_bytes(n_box));
  // an interleaved stereo pair: both channels of a sample in one aligned 8-byte load
  const bool pair = xR == xL + 1 && x_stride == 2 && ((uintptr_t)xL & 7) == 0;
  launch_pan_offsets(boxes, n_box, scratch, s);
  if (n_items > 0) {
    rc = dispatch_logh<3, 13>(ilog2(H), [&](auto lh) {
      return dispatch_bool(pair, [&](auto pr) {
        using G = FftGeom<decltype(lh)::value>;
        // beside the frames: the waves' partial sums and counts (frame_lane_sum)
        return launch_with_lds(k_stft_pan<decltype(lh)::value, decltype(pr)::value>, dim3(G::grid(n_items)), dim3(G::Threads),
                               G::FramesLds + (size_t)G::Threads / kWave * 16, device, s, xL, xR, n, x_stride, n_fft, hop, window, tw.w,
                               tw.post, boxes, n_box, offs, part, n_items, scale);
      });
    });
    if (rc != PAR_OK) return rc;
  }
  launch_pan_reduce(n_box, scratch, fac, count, s);
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}

// Time-averaged dB spectra of all channels straight from the samples (k_stft_mean + k_mean_db_reduce): what
// par_mean_db_frames_f32 sums over the mode-1 spectrogram of each channel, divided by the frame count, without the spectrogram.
size_t par_stft_mean_db_scratch_bytes(int64_t n, int n_fft, int hop, int zeropad, int n_ch) {
  if (n < 1 || hop < 1 || n_ch < 1 || n_ch > 8 || !stft_size_supported(n_fft, zeropad)) return 0;
  const int64_t n_frames = par_stft_frames(n, n_fft, hop);
  const int64_t n_runs = par::ceil_div(n_frames, par::mean_run_len(n_frames));
  return (size_t)n_ch * (size_t)n_runs * (size_t)((int64_t)n_fft * zeropad / 2 + 1) * sizeof(double);
}

int par_stft_mean_db_f32(int device, const float* x, int64_t n, int64_t x_stride, int n_ch, int n_fft, int hop, int zeropad,
                         const float* window, double* mean, void* scratch, size_t scratch_bytes, void* stream) {
  using namespace par;
  PAR_REQUIRE(x && window && mean && scratch, PAR_ERR_ARG, "par_stft_mean_db_f32: null pointer");
  PAR_REQUIRE(n >= 1 && hop >= 1 && zeropad >= 1 && n_fft >= 2 && n_ch >= 1 && n_ch <= 8 && x_stride >= n_ch, PAR_ERR_ARG,
              "par_stft_mean_db_f32: bad sizes (n %lld, n_fft %d, hop %d, zeropad %d, channels %d, stride %lld)", (long long)n, n_fft, hop,
              zeropad, n_ch, (long long)x_stride);
  PAR_REQUIRE(((uintptr_t)scratch & 7) == 0 && ((uintptr_t)mean & 7) == 0, PAR_ERR_ARG, "par_stft_mean_db_f32: mean or scratch is not 8-byte aligned");
  int rc = require_stft_size("par_stft_mean_db_f32", n_fft, zeropad);
  if (rc != PAR_OK) return rc;
  const size_t need = par_stft_mean_db_scratch_bytes(n, n_fft, hop, zeropad, n_ch);
  PAR_REQUIRE(scratch_bytes >= need, PAR_ERR_WORKSPACE, "par_stft_mean_db_f32: scratch %zu < %zu", scratch_bytes, need);
  const int M = n_fft * zeropad, H = M / 2;
  const int64_t n_frames = par_stft_frames(n, n_fft, hop);
  const int64_t run = mean_run_len(n_frames), n_runs = ceil_div(n_frames, run);
  PAR_HIP_CHECK(hipSetDevice(device));
  Twiddles tw;
  rc = get_twiddles(device, M, &tw);
  if (rc != PAR_OK) return rc;
  hipStream_t s = as_stream(stream);
  const float scale = (float)(1.0 / sqrt((double)n_fft));
  double* part = reinterpret_cast<double*>(scratch);
  rc = dispatch_logh<3, 13>(ilog2(H), [&](auto lh) {
    return dispatch_bool(x_stride == 1, [&](auto unit) {
      using G = FftGeom<decltype(lh)::value>;
      return launch_with_lds(k_stft_mean<decltype(lh)::value, decltype(unit)::value>, dim3(G::grid(n_runs), (unsigned)n_ch), dim3(G::Threads),
                             G::FramesLds, device, s, x, n, x_stride, n_fft, hop, window, tw.w, tw.post, part, n_frames, run, n_runs, scale);
    });
  });
  if (rc != PAR_OK) return rc;
  const int bins = H + 1;
  hipLaunchKernelGGL(k_mean_db_reduce, dim3((unsigned)ceil_div(bins, 256), (unsigned)n_ch), dim3(256), 0, s, part, n_runs, bins, n_frames, mean);
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}

// Spectrogram image straight from the samples (k_image_plan + k_image_zero + k_stft_peak_image): what par_peak_image_f32 takes
// from the mode-1 spectrogram of x, without the spectrogram.
size_t par_stft_peak_image_scratch_bytes(int64_t width) {
  if (width < 1 || width > par::kImageMaxSide) return 0;
  return (size_t)(width + 1) * sizeof(int64_t);
}

int par_stft_peak_image_f32(int device, const float* x, int64_t n, int64_t x_stride, int n_fft, int hop, int zeropad,
                            const float* window, const int64_t* cols, const int64_t* cols_host, const int32_t* rows,
                            const int32_t* rows_host, int64_t width, int64_t height, float* peak, int64_t pitch, void* scratch,
                            size_t scratch_bytes, void* stream) {
  using namespace par;
  PAR_REQUIRE(x && window && cols && cols_host && rows && rows_host && peak && scratch, PAR_ERR_ARG, "par_stft_peak_image_f32: null pointer");
  PAR_REQUIRE(n >= 1 && x_stride >= 1 && hop >= 1 && zeropad >= 1 && n_fft >= 2 && width >= 1 && height >= 1 && width <= kImageMaxSide &&
                  height <= kImageMaxSide && pitch >= height,
              PAR_ERR_ARG, "par_stft_peak_image_f32: bad sizes (n %lld, stride %lld, n_fft %d, hop %d, zeropad %d, image %lld x %lld, pitch %lld)",
              (long long)n, (long long)x_stride, n_fft, hop, zeropad, (long long)width, (long long)height, (long long)pitch);
  PAR_REQUIRE(((uintptr_t)scratch & 7) == 0, PAR_ERR_ARG, "par_stft_peak_image_f32: scratch is not 8-byte aligned");
  int rc = require_stft_size("par_stft_peak_image_f32", n_fft, zeropad);
  if (rc != PAR_OK) return rc;
  const int M = n_fft * zeropad, H = M / 2;
  const int64_t n_frames = par_stft_frames(n, n_fft, hop);
  ImagePlan plan;
  rc = image_check_tables("par_stft_peak_image_f32", cols_host, rows_host, width, height, n_frames, H + 1, &plan);
  if (rc != PAR_OK) return rc;
  const size_t need = par_stft_peak_image_scratch_bytes(width);
  PAR_REQUIRE(scratch_bytes >= need, PAR_ERR_WORKSPACE, "par_stft_peak_image_f32: scratch %zu < %zu", scratch_bytes, need);
  PAR_HIP_CHECK(hipSetDevice(device));
  Twiddles tw;
  rc = get_twiddles(device, M, &tw);
  if (rc != PAR_OK) return rc;
  hipStream_t s = as_stream(stream);
  const float scale = (float)(1.0 / sqrt((double)n_fft));
  int64_t* unit_off = reinterpret_cast<int64_t*>(scratch);
  hipLaunchKernelGGL(k_image_zero, dim3((unsigned)width, (unsigned)ceil_div(height, 256)), dim3(256), 0, s, peak, width, (int)height, pitch);
  PAR_HIP_CHECK(hipGetLastError());
  if (plan.n_units == 0) return PAR_OK;
  hipLaunchKernelGGL(k_image_plan, dim3(1), dim3(1024), 0, s, cols, width, plan.chunk, n_frames, unit_off);
  PAR_HIP_CHECK(hipGetLastError());
  return dispatch_logh<3, 13>(ilog2(H), [&](auto lh) {
    return dispatch_bool(x_stride == 1, [&](auto unit) {
      using G = FftGeom<decltype(lh)::value>;
      return launch_with_lds(k_stft_peak_image<decltype(lh)::value, decltype(unit)::value>, dim3(G::grid(plan.n_units)), dim3(G::Threads),
                             G::FramesLds, device, s, x, n, x_stride, n_fft, hop, window, tw.w, tw.post, cols, rows,
                             (const int64_t*)unit_off, width, (int)height, peak, pitch, n_frames, plan.chunk, plan.passes, plan.n_units, scale);
    });
  });
}

// Peak / Peak Track straight from the samples (k_stft_peak): what par_track_peak_f64 traces on the mode-1 spectrogram of x
// (db: on its float32 dB), without the spectrogram.
int par_stft_track_peak_f64(int device, const float* x, int64_t n, int64_t x_stride, int n_fft, int hop, int zeropad,
                            const float* window, int64_t frame_0, int64_t count, double* freqs, double sr,
                            double tolerance_oct, int mode, int db, int32_t* status, void* stream) {
  using namespace par;
  PAR_REQUIRE(x && window && freqs && status, PAR_ERR_ARG, "par_stft_track_peak_f64: null pointer");
  PAR_REQUIRE(n >= 1 && x_stride >= 1 && hop >= 1 && zeropad >= 1 && n_fft >= 2, PAR_ERR_ARG,
              "par_stft_track_peak_f64: bad sizes (n %lld, stride %lld, n_fft %d, hop %d, zeropad %d)", (long long)n, (long long)x_stride,
              n_fft, hop, zeropad);
  PAR_REQUIRE(count >= 0 && frame_0 >= 0 && count <= par_stft_frames(n, n_fft, hop) && frame_0 <= par_stft_frames(n, n_fft, hop) - count,
              PAR_ERR_ARG, "par_stft_track_peak_f64: frames [%lld, %lld + %lld) of %lld", (long long)frame_0, (long long)frame_0,
              (long long)count, (long long)par_stft_frames(n, n_fft, hop));
  PAR_REQUIRE((mode == 0 || mode == 1) && (db == 0 || db == 1), PAR_ERR_ARG, "par_stft_track_peak_f64: mode and db must be 0 or 1");
  int rc = require_stft_size("par_stft_track_peak_f64", n_fft, zeropad);
  if (rc != PAR_OK) return rc;
  if (count == 0) return PAR_OK;
  const int M = n_fft * zeropad, H = M / 2;
  PAR_HIP_CHECK(hipSetDevice(device));
  Twiddles tw;
  rc = get_twiddles(device, M, &tw);
  if (rc != PAR_OK) return rc;
  hipStream_t s = as_stream(stream);
  PAR_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), s));
  double centre = 0.0;
  if (mode == 1) {                                           // the band of every frame sits on the first trail frequency
    PAR_HIP_CHECK(hipMemcpyAsync(&centre, freqs, sizeof(double), hipMemcpyDeviceToHost, s));
    PAR_HIP_CHECK(hipStreamSynchronize(s));
  }
  const float scale = (float)(1.0 / sqrt((double)n_fft));
  rc = dispatch_logh<3, 13>(ilog2(H), [&](auto lh) {
    return dispatch_bool(x_stride == 1, [&](auto unit) {
      using G = FftGeom<decltype(lh)::value>;
      // the frames, then per frame 4 ints of band and one (value, bin) pair per wave of the frame
      return launch_with_lds(k_stft_peak<decltype(lh)::value, decltype(unit)::value>, dim3(G::grid(count)), dim3(G::Threads),
                             G::FramesLds + (size_t)G::Frames * (4 + 2 * (G::T > kWave ? G::T / kWave : 1)) * sizeof(int), device, s, x, n,
                             x_stride, n_fft, hop, window, tw.w, tw.post, frame_0, count, freqs, centre, sr, tolerance_oct, mode, db,
                             status, scale);
    });
  });
  if (rc != PAR_OK) return rc;
  return check_empty(status, s, "par_stft_track_peak_f64");
}

// Frames of more than 8192 points (up to 2^21): four-step transform through a caller-owned scratch of
// par_stft_big_scratch_bytes() (one H-point complex array per frame of a batch; a batch fills up to 1 GiB).
size_t par_stft_big_scratch_bytes(int64_t n, int n_fft, int hop, int zeropad) {
  const int64_t M = (int64_t)n_fft * zeropad;
  if (M > (1ll << 21) && M <= (1ll << 24)) return (size_t)(2 * (M / 2) * (int64_t)sizeof(float2));   // z_r and Z_r of ONE frame
  if (M <= 8192 || M > (1ll << 21)) return 0;
  // frames per batch: as many as fit 1 GiB of scratch (at least 16, at most what one grid dimension takes): 16-frame
  // batches made the 16384-point transform launch-bound (880 batches of three small launches: 16 ms for a 10-minute file)
  int64_t frames = par_stft_frames(n, n_fft, hop);
  const int64_t per_frame = (M / 2) * (int64_t)sizeof(float2);       // A[k1][n2]; the row pass writes the bins itself
  int64_t cap = (1ll << 30) / per_frame;
  cap = cap < 16 ? 16 : (cap > 32768 ? 32768 : cap);
  if (frames > cap) frames = cap;
  return (size_t)(frames * per_frame);
}

int par_stft_big_f32(int device, const float* x, int64_t n, int64_t x_stride, int n_fft, int hop, int zeropad,
                     const float* window, float* out, int mode, void* scratch, size_t scratch_bytes, void* stream) {
  using namespace par;
  PAR_REQUIRE(x && window && out && scratch, PAR_ERR_ARG, "par_stft_big_f32: null pointer");
  PAR_REQUIRE(n >= 1 && x_stride >= 1 && hop >= 1 && zeropad >= 1 && n_fft >= 2, PAR_ERR_ARG, "par_stft_big_f32: bad sizes");
  PAR_REQUIRE(mode == 0 || mode == 1, PAR_ERR_ARG, "par_stft_big_f32: mode must be 0 (complex) or 1 (magnitude)");
  const int64_t M64 = (int64_t)n_fft * zeropad;
  PAR_REQUIRE(M64 > 8192 && M64 <= (1ll << 24) && (M64 & (M64 - 1)) == 0 && (n_fft % 2) == 0, PAR_ERR_UNSUPPORTED,
              "par_stft_big_f32: n_fft*zeropad=%lld is not a power of two in (8192, 2^24]", (long long)M64);
  PAR_REQUIRE(scratch_bytes >= par_stft_big_scratch_bytes(n, n_fft, hop, zeropad), PAR_ERR_WORKSPACE,
              "par_stft_big_f32: scratch %zu < %zu", scratch_bytes, par_stft_big_scratch_bytes(n, n_fft, hop, zeropad));
  PAR_HIP_CHECK(hipSetDevice(device));
  hipStream_t s = as_stream(stream);
  const int64_t H = M64 / 2;
  if (M64 > (1ll << 21)) {
    // 2^22 .. 2^24 points: R = H / 2^20 decimated sequences of 2^20 points through the four-step transform, recombined and
    // untangled bin by bin (k_huge_gather / k_huge_out), a frame at a time
    const int64_t Hp = 1ll << 20;
    int logR = 0;
    while ((Hp << logR) < H) ++logR;
    float2* z = static_cast<float2*>(scratch);
    float2* Z = z + H;
    const int64_t frames = par_stft_frames(n, n_fft, hop);
    const float scale_h = (float)(1.0 / sqrt((double)n_fft));
    for (int64_t f = 0; f < frames; ++f) {
      hipLaunchKernelGGL(k_huge_gather, dim3((unsigned)ceil_div(H, 256)), dim3(256), 0, s, x, n, x_stride, n_fft, hop, window, f, logR,
                         Hp, z);
      const int rc = big_fft_c2c(device, z, Z, Hp, (int64_t)1 << logR, s);
      if (rc != PAR_OK) return rc;
      if (mode == 0)
        hipLaunchKernelGGL(k_huge_out<0>, dim3((unsigned)ceil_div(Hp, 256)), dim3(256), 0, s, (const float2*)Z, logR, Hp, out,
                           f * (H + 1), scale_h);
      else
        hipLaunchKernelGGL(k_huge_out<1>, dim3((unsigned)ceil_div(Hp, 256)), dim3(256), 0, s, (const float2*)Z, logR, Hp, out,
                           f * (H + 1), scale_h);
    }
    PAR_HIP_CHECK(hipGetLastError());
    return PAR_OK;
  }
  // N1 >= N2, both in [64, 1024]: the balanced split, except 2^15 = 512 x 64 -- both pure radix-8 sizes (five radix-8 stages
  // instead of 256 x 128's four plus a radix-4 and a radix-2 stage) -- and 2^14 = 256 x 64 (one remainder stage instead of two)
  const int L = ilog2((int)H), l1 = L == 15 ? 9 : (L == 14 ? 8 : (L + 1) / 2), l2 = L - l1;
  Twiddles t1, t2;
  BigTw bt;
  int rc = get_twiddles(device, 2 << l1, &t1);
  if (rc == PAR_OK) rc = get_twiddles(device, 2 << l2, &t2);
  BigTw bt2;                                                              // the untangle step's half-step circle
  if (rc == PAR_OK) rc = get_big_twiddles(device, (int)H, &bt);
  if (rc == PAR_OK) rc = get_big_twiddles(device, (int)(2 * H), &bt2);
  if (rc != PAR_OK) return rc;
  const int64_t n_frames = par_stft_frames(n, n_fft, hop);
  const float scale = (float)(1.0 / sqrt((double)n_fft));
  float2* A = static_cast<float2*>(scratch);
  // frames the scratch holds: one H-point array per frame
  int64_t batch = (int64_t)(scratch_bytes / (size_t)(H * (int64_t)sizeof(float2)));
  batch = batch > 32768 ? 32768 : batch;
  for (int64_t f0 = 0; f0 < n_frames; f0 += batch) {
    const int64_t nb = n_frames - f0 < batch ? n_frames - f0 : batch;
#define PAR_BIG_COLS(LS, NG, TW)                                                                                         \
  if (int rc_lds = raise_dynamic_lds(reinterpret_cast<const void*>(&k_bigfft<LS, 0>),                                    \
                                     kBigC * ((1 << LS) + (1 << LS) / 8 + 8) * (int)sizeof(float2), device))             \
    return rc_lds;                                                                                                       \
  hipLaunchKernelGGL((k_bigfft<LS, 0>), dim3((unsigned)round_up8((int64_t)((NG) / kBigC) * nb)), dim3(1 << LS),           \
                     (size_t)kBigC * ((1 << LS) + (1 << LS) / 8 + 8) * sizeof(float2), s, x, n, x_stride, n_fft, hop,     \
                     window, TW, bt.lo, bt.hi, A, (float2*)nullptr, f0, l1, l2, nb)
    switch (l1) {
      case 7: PAR_BIG_COLS(7, 1 << l2, t1.w); break;
      case 8: PAR_BIG_COLS(8, 1 << l2, t1.w); break;
      case 9: PAR_BIG_COLS(9, 1 << l2, t1.w); break;
      case 10: PAR_BIG_COLS(10, 1 << l2, t1.w); break;
      default: PAR_REQUIRE(false, PAR_ERR_UNSUPPORTED, "par_stft_big_f32: unsupported size");
    }
#undef PAR_BIG_COLS
    // rows + untangle: 16 padded spectra in LDS (148 KB at 1024 points: above the 64 KB default)
#define PAR_BIG_ROWS(LS)                                                                                                 \
  {                                                                                                                      \
    constexpr int kLds = 2 * kBigC * ((1 << LS) + (1 << LS) / 8 + 8) * (int)sizeof(float2);                              \
    int rc_lds = raise_dynamic_lds(reinterpret_cast<const void*>(&k_bigfft_rows_out<LS, 0>), kLds, device);              \
    if (rc_lds == PAR_OK) rc_lds = raise_dynamic_lds(reinterpret_cast<const void*>(&k_bigfft_rows_out<LS, 1>), kLds, device); \
    if (rc_lds != PAR_OK) return rc_lds;                                                                                 \
    const dim3 grid((unsigned)round_up8((int64_t)((1 << l1) / (2 * kBigC) + 1) * nb));                                   \
    if (mode == 0)                                                                                                       \
      hipLaunchKernelGGL((k_bigfft_rows_out<LS, 0>), grid, dim3(1 << LS), kLds, s, (const float2*)A, t2.w, bt2.lo, bt2.hi, out, \
                         f0, l1, scale, nb);                                                                               \
    else                                                                                                                 \
      hipLaunchKernelGGL((k_bigfft_rows_out<LS, 1>), grid, dim3(1 << LS), kLds, s, (const float2*)A, t2.w, bt2.lo, bt2.hi, out, \
                         f0, l1, scale, nb);                                                                               \
  }
    switch (l2) {
      case 6: PAR_BIG_ROWS(6); break;
      case 7: PAR_BIG_ROWS(7); break;
      case 8: PAR_BIG_ROWS(8); break;
      case 9: PAR_BIG_ROWS(9); break;
      case 10: PAR_BIG_ROWS(10); break;
      default: PAR_REQUIRE(false, PAR_ERR_UNSUPPORTED, "par_stft_big_f32: unsupported size");
    }
#undef PAR_BIG_ROWS
    PAR_HIP_CHECK(hipGetLastError());
  }
  return PAR_OK;
}

// X2: xcorr(a, b, 'full') of two float64 device signals (util/correlation.py:6-13): full[na + nb - 1] float64 out.
// scratch: par_xcorr_scratch_bytes(na, nb) device bytes.  The values carry the float32 transform's error (~1e-6 of the
// peak); par_find_delay_f64 refines what the tape-sync tool needs exactly.
constexpr int64_t kXcMaxFft = 1ll << 20;         // the four-step transform's largest size
constexpr int64_t kXcSection = kXcMaxFft / 2;    // longer signals are correlated section pair by section pair
constexpr int64_t kXcMaxLen = 1ll << 25;         // per signal (4096 section pairs of two 2^20-point transforms each)
static int64_t xc_fft_len(int64_t na, int64_t nb) {
  int64_t N = 8192;
  while (N < na + nb - 1 && N < kXcMaxFft) N <<= 1;
  return N;
}
// The single pair's scratch: Z[N] | Y[N] | 64 bytes | full[na + nb - 1] | the row record | the search's results | spare.
// The sizes are the ABI's (callers allocate by par_xcorr_scratch_bytes): the row and the results live in the kXcSpare
// doubles that have always followed the lags.
constexpr int64_t kXcSpare = 16 + 2 * par::kXcCand + 8;
struct XcResult {                                // what par_find_delay_f64 copies to the host, once
  double delay, corr;
  int32_t status, pad;
};
static_assert(sizeof(par::XcbRow) + sizeof(XcResult) <= (size_t)kXcSpare * sizeof(double) && alignof(par::XcbRow) <= sizeof(double),
              "the single call's row record and results must fit the spare doubles of par_xcorr_scratch_bytes");
size_t par_xcorr_scratch_bytes(int64_t na, int64_t nb) {
  if (na < 1 || nb < 1) return 0;
  return (size_t)(2 * xc_fft_len(na, nb) * sizeof(float2) + 64 + (size_t)(na + nb + kXcSpare) * sizeof(double));
}
struct XcScratch {
  float2 *Z, *Y;
  double* full;
  par::XcbRow* row;
  XcResult* res;
};
static XcScratch xc_scratch(void* scratch, int64_t N, int64_t na, int64_t nb) {
  XcScratch sc;
  sc.Z = static_cast<float2*>(scratch);
  sc.Y = sc.Z + N;
  sc.full = reinterpret_cast<double*>(reinterpret_cast<char*>(sc.Y + N) + 64);
  sc.row = reinterpret_cast<par::XcbRow*>(sc.full + (na + nb - 1));
  sc.res = reinterpret_cast<XcResult*>(sc.row + 1);
  return sc;
}

// The correlation of one pair as a batch of one row: norms into the row record, then pack -> transform -> cross spectrum
// -> transform -> `full`, section pair by section pair where one transform does not hold the lags.
static int xcorr_full(int device, const double* a, int64_t na, const double* b, int64_t nb, const XcScratch& sc, double* full,
                      hipStream_t s) {
  using namespace par;
  const int64_t N = xc_fft_len(na, nb);
  PAR_REQUIRE(na <= kXcMaxLen && nb <= kXcMaxLen, PAR_ERR_UNSUPPORTED, "xcorr: %lld / %lld samples (limit 2^25 per signal)",
              (long long)na, (long long)nb);
  float2 *Z = sc.Z, *Y = sc.Y;
  const dim3 gN((unsigned)ceil_div(N, 256));
  hipLaunchKernelGGL(k_xcb_norms, dim3(2), dim3(1024), 0, s, a, na, na, b, nb, nb, sc.row);
  if (na + nb - 1 > N) {
    // Windows of more than ~2.7 s at 192 kHz: correlation is bilinear, so the signals are cut into sections of 2^19
    // samples and every pair (p, q) adds its 2^20-point correlation into full at the lag offset p - q sections.  The
    // float32 transforms only have to FIND the peak; par_find_delay_f64 re-evaluates the lags around it exactly.
    PAR_HIP_CHECK(hipMemsetAsync(full, 0, (size_t)(na + nb - 1) * sizeof(double), s));
    for (int64_t pa = 0; pa < na; pa += kXcSection) {
      const int64_t la = na - pa < kXcSection ? na - pa : kXcSection;
      for (int64_t qb = 0; qb < nb; qb += kXcSection) {
        const int64_t lb = nb - qb < kXcSection ? nb - qb : kXcSection;
        hipLaunchKernelGGL(k_xcb_pack, gN, dim3(256), 0, s, a + pa, la, la, b + qb, lb, lb, (const XcbRow*)sc.row, Z, N);
        int rc = big_fft_c2c(device, Z, Y, N, 1, s);
        if (rc != PAR_OK) return rc;
        hipLaunchKernelGGL(k_xcb_cross, gN, dim3(256), 0, s, (const float2*)Y, Z, N);
        rc = big_fft_c2c(device, Z, Y, N, 1, s);
        if (rc != PAR_OK) return rc;
        // local index jl = lag + lb - 1; global index = lag + (pa - qb) + nb - 1
        const int64_t joff = pa - qb + nb - lb;
        hipLaunchKernelGGL(k_xc_unpack_acc, dim3((unsigned)ceil_div(la + lb - 1, 256)), dim3(256), 0, s, (const float2*)Y, N, lb,
                           la + lb - 1, full + joff);
      }
    }
    PAR_HIP_CHECK(hipGetLastError());
    return PAR_OK;
  }
  hipLaunchKernelGGL(k_xcb_pack, gN, dim3(256), 0, s, a, na, na, b, nb, nb, (const XcbRow*)sc.row, Z, N);
  int rc = big_fft_c2c(device, Z, Y, N, 1, s);                       // Y = FFT(a + i b)
  if (rc != PAR_OK) return rc;
  hipLaunchKernelGGL(k_xcb_cross, gN, dim3(256), 0, s, (const float2*)Y, Z, N);
  rc = big_fft_c2c(device, Z, Y, N, 1, s);                           // Y = conj(N * circular correlation)
  if (rc != PAR_OK) return rc;
  hipLaunchKernelGGL(k_xc_unpack, dim3((unsigned)ceil_div(na + nb - 1, 256)), dim3(256), 0, s, (const float2*)Y, N, nb,
                     na + nb - 1, full);
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}

int par_xcorr_f64(int device, const double* a, int64_t na, const double* b, int64_t nb, void* scratch, size_t scratch_bytes,
                  double* full, void* stream) {
  using namespace par;
  PAR_REQUIRE(a && b && scratch && full && na >= 1 && nb >= 1, PAR_ERR_ARG, "par_xcorr_f64: bad args");
  PAR_REQUIRE(scratch_bytes >= par_xcorr_scratch_bytes(na, nb), PAR_ERR_WORKSPACE, "par_xcorr_f64: scratch too small");
  PAR_HIP_CHECK(hipSetDevice(device));
  return xcorr_full(device, a, na, b, nb, xc_scratch(scratch, xc_fft_len(na, nb), na, nb), full, as_stream(stream));
}

// find_delay(a, b, ignore_phase) of util/correlation.py:16-39 (windows are applied by the caller, in place, like the
// reference): *delay = parabola-refined peak of the 'same' correlation minus len//2, *corr = its height.  The peak is
// located by the float32 transform and the lags around it are re-evaluated as float64 dot products.  A peak on the last
// lag is the reference's IndexError (PAR_ERR_INDEX).  The batch of one row, with one difference in where the peak stage
// reads: a batch row's lags come straight out of its transform (at most 2^20 of them, one 256-thread workgroup per row);
// here ONE workgroup has up to 2^26 lags to scan, so the lags are first formed as the float64 'full' array by a full grid
// (sums over section pairs in the sectioned form) and scanned by 1024 threads.  The doubles compared are the same.
// Synchronises once, for the copy of delay, corr and status to the host.
int par_find_delay_f64(int device, const double* a, int64_t na, const double* b, int64_t nb, int ignore_phase, void* scratch,
                       size_t scratch_bytes, double* delay, double* corr, void* stream) {
  using namespace par;
  PAR_REQUIRE(a && b && scratch && delay && corr && na >= 3 && nb >= 1, PAR_ERR_ARG, "par_find_delay_f64: bad args");
  PAR_REQUIRE(scratch_bytes >= par_xcorr_scratch_bytes(na, nb), PAR_ERR_WORKSPACE, "par_find_delay_f64: scratch too small");
  PAR_HIP_CHECK(hipSetDevice(device));
  hipStream_t s = as_stream(stream);
  const XcScratch sc = xc_scratch(scratch, xc_fft_len(na, nb), na, nb);
  const int rc = xcorr_full(device, a, na, b, nb, sc, sc.full, s);
  if (rc != PAR_OK) return rc;
  xc_search<XcLagsOfFull, 1024>(XcLagsOfFull{sc.full}, a, na, na, b, nb, nb, 1, ignore_phase, sc.row, &sc.res->delay, &sc.res->corr,
                                &sc.res->status, s);
  PAR_HIP_CHECK(hipGetLastError());
  XcResult r;
  PAR_HIP_CHECK(hipMemcpyAsync(&r, sc.res, sizeof(r), hipMemcpyDeviceToHost, s));
  PAR_HIP_CHECK(hipStreamSynchronize(s));
  PAR_REQUIRE(r.status != 1, PAR_ERR_INDEX, "par_find_delay_f64: correlation peak on the last lag (index %lld is out of bounds "
              "for axis 0 with size %lld in the reference's parabolic())", (long long)na, (long long)na);
  *delay = r.delay;
  *corr = r.corr;
  return PAR_OK;
}

// X2 batch: find_delay for n_win pairs of rows (a[w * a_pitch ..], b[w * b_pitch ..]) of one shape (na, nb), every window
// decided on the device (the kernels above).  Windows are processed in passes of as many as scratch_bytes holds: per window
// two N-point complex arrays and one XcbRow.  Nothing synchronises here but big_fft_c2c's table upload on a device's
// first call of a size.
constexpr size_t kXcbCap = (size_t)1 << 30;        // transform arrays of one pass
constexpr int64_t kXcbMaxPass = 32768;             // windows of one pass (the y extent of a grid)
static size_t xcb_window_bytes(int64_t N) { return (size_t)(2 * N) * sizeof(float2) + sizeof(par::XcbRow); }
size_t par_find_delay_batch_scratch_bytes(int64_t na, int64_t nb, int64_t n_win) {
  if (na < 1 || nb < 1 || na + nb - 1 > kXcMaxFft) return 0;
  const int64_t N = xc_fft_len(na, nb);
  int64_t fit = (int64_t)(kXcbCap / ((size_t)(2 * N) * sizeof(float2)));
  if (fit > kXcbMaxPass) fit = kXcbMaxPass;
  int64_t c = n_win < 1 ? 1 : n_win;
  if (c > fit) c = fit;
  return (size_t)c * xcb_window_bytes(N);
}
int par_find_delay_batch_f64(int device, double* a, int64_t a_pitch, int64_t na, double* b, int64_t b_pitch, int64_t nb,
                             int64_t n_win, const double* win_a, const double* win_b, int ignore_phase, void* scratch,
                             size_t scratch_bytes, double* delay, double* corr, int32_t* status, void* stream) {
  using namespace par;
  PAR_REQUIRE(a && b && scratch && delay && corr && status, PAR_ERR_ARG, "par_find_delay_batch_f64: null pointer");
  PAR_REQUIRE(na >= 3 && nb >= 1 && n_win >= 0, PAR_ERR_ARG, "par_find_delay_batch_f64: na %lld (>= 3), nb %lld (>= 1), n_win %lld (>= 0)",
              (long long)na, (long long)nb, (long long)n_win);
  PAR_REQUIRE(a_pitch >= na && b_pitch >= nb, PAR_ERR_ARG, "par_find_delay_batch_f64: pitch %lld / %lld below the row length %lld / %lld",
              (long long)a_pitch, (long long)b_pitch, (long long)na, (long long)nb);
  if (n_win == 0) return PAR_OK;
  PAR_REQUIRE(na + nb - 1 <= kXcMaxFft, PAR_ERR_UNSUPPORTED,
              "par_find_delay_batch_f64: %lld + %lld - 1 lags need the sectioned form, which is not batched (limit 2^20)", (long long)na,
              (long long)nb);
  const int64_t N = xc_fft_len(na, nb);
  int64_t C = (int64_t)(scratch_bytes / xcb_window_bytes(N));
  PAR_REQUIRE(C >= 1, PAR_ERR_WORKSPACE, "par_find_delay_batch_f64: scratch holds less than one window (%zu bytes)", xcb_window_bytes(N));
  if (C > kXcbMaxPass) C = kXcbMaxPass;
  if (C > n_win) C = n_win;
  PAR_HIP_CHECK(hipSetDevice(device));
  hipStream_t s = as_stream(stream);
  float2* Z = static_cast<float2*>(scratch);
  float2* Y = Z + C * N;
  XcbRow* rows = reinterpret_cast<XcbRow*>(Y + C * N);
  const int64_t nmax = na > nb ? na : nb;
  for (int64_t w0 = 0; w0 < n_win; w0 += C) {
    const int64_t c = n_win - w0 < C ? n_win - w0 : C;
    double* ac = a + w0 * a_pitch;
    double* bc = b + w0 * b_pitch;
    const dim3 gN((unsigned)ceil_div(N, 256), (unsigned)c);
    if (win_a || win_b)
      hipLaunchKernelGGL(k_xcb_window, dim3((unsigned)ceil_div(nmax, 256), (unsigned)c), dim3(256), 0, s, ac, a_pitch, na, bc, b_pitch, nb,
                         win_a, win_b);
    hipLaunchKernelGGL(k_xcb_norms, dim3(2, (unsigned)c), dim3(1024), 0, s, (const double*)ac, a_pitch, na, (const double*)bc, b_pitch,
                       nb, rows);
    hipLaunchKernelGGL(k_xcb_pack, gN, dim3(256), 0, s, (const double*)ac, a_pitch, na, (const double*)bc, b_pitch, nb,
                       (const XcbRow*)rows, Z, N);
    int rc = big_fft_c2c(device, Z, Y, N, c, s);                        // Y = FFT(a + i b), window by window
    if (rc != PAR_OK) return rc;
    hipLaunchKernelGGL(k_xcb_cross, gN, dim3(256), 0, s, (const float2*)Y, Z, N);
    rc = big_fft_c2c(device, Z, Y, N, c, s);                            // Y = conj(N * circular correlation)
    if (rc != PAR_OK) return rc;
    xc_search<XcLagsOfY, 256>(XcLagsOfY{Y, N}, ac, a_pitch, na, bc, b_pitch, nb, c, ignore_phase, rows, delay + w0, corr + w0, status + w0,
                              s);
    PAR_HIP_CHECK(hipGetLastError());
  }
  return PAR_OK;
}

// X2 sectioned batch: find_delay for n_win pairs of read-only rows of ANY length up to 2^25 (experiments/group_delay.py
// correlates whole files, band by band): see include/par_hip.h.  Per row of a pass two arrays of D N complex values and
// one XcbRow; the kernels are k_xcs_* above, the transforms big_fft_c2c, the search xc_search.
struct XcsShape {
  int64_t S, N;
  int P, Q, M, D;
};
static bool xcs_shape(int64_t na, int64_t nb, int section_log2, XcsShape* sh) {
  if (na < 1 || nb < 1 || na > kXcMaxLen || nb > kXcMaxLen || !(section_log2 == 0 || (section_log2 >= 12 && section_log2 <= 19)))
    return false;
  sh->S = (int64_t)1 << (section_log2 ? section_log2 : 19);
  sh->N = 2 * sh->S;
  sh->P = (int)((na + sh->S - 1) / sh->S);
  sh->Q = (int)((nb + sh->S - 1) / sh->S);
  sh->M = sh->P > sh->Q ? sh->P : sh->Q;
  sh->D = sh->P + sh->Q - 1;
  return true;
}
static size_t xcs_row_bytes(const XcsShape& sh) { return (size_t)(2 * sh.D * sh.N) * sizeof(float2) + sizeof(par::XcbRow); }
size_t par_find_delay_sect_scratch_bytes(int64_t na, int64_t nb, int64_t n_win, int section_log2) {
  XcsShape sh;
  if (!xcs_shape(na, nb, section_log2, &sh)) return 0;
  int64_t fit = (int64_t)(kXcbCap / ((size_t)(2 * sh.D * sh.N) * sizeof(float2)));
  if (fit > kXcbMaxPass) fit = kXcbMaxPass;
  if (fit < 1) fit = 1;
  int64_t c = n_win < 1 ? 1 : n_win;
  if (c > fit) c = fit;
  return (size_t)c * xcs_row_bytes(sh);
}
int par_find_delay_sect_f64(int device, const double* a, int64_t a_pitch, int64_t na, const double* b, int64_t b_pitch, int64_t nb,
                            int64_t n_win, int section_log2, int ignore_phase, void* scratch, size_t scratch_bytes, double* delay,
                            double* corr, int32_t* status, double* norms, double* same_out, int64_t same_pitch, void* stream) {
  using namespace par;
  PAR_REQUIRE(a && b && scratch && delay && corr && status, PAR_ERR_ARG, "par_find_delay_sect_f64: null pointer");
  PAR_REQUIRE(na >= 3 && nb >= 1 && n_win >= 0, PAR_ERR_ARG, "par_find_delay_sect_f64: na %lld (>= 3), nb %lld (>= 1), n_win %lld (>= 0)",
              (long long)na, (long long)nb, (long long)n_win);
  PAR_REQUIRE(a_pitch >= na && b_pitch >= nb && (!same_out || same_pitch >= na), PAR_ERR_ARG,
              "par_find_delay_sect_f64: pitch %lld / %lld / %lld below the row length %lld / %lld / %lld", (long long)a_pitch,
              (long long)b_pitch, (long long)same_pitch, (long long)na, (long long)nb, (long long)na);
  PAR_REQUIRE(section_log2 == 0 || (section_log2 >= 12 && section_log2 <= 19), PAR_ERR_ARG,
              "par_find_delay_sect_f64: section_log2 %d outside {0, 12..19}", section_log2);
  if (n_win == 0) return PAR_OK;
  PAR_REQUIRE(na <= kXcMaxLen && nb <= kXcMaxLen, PAR_ERR_UNSUPPORTED, "par_find_delay_sect_f64: %lld / %lld samples (limit 2^25 per row)",
              (long long)na, (long long)nb);
  XcsShape sh;
  xcs_shape(na, nb, section_log2, &sh);
  int64_t Cp = (int64_t)(scratch_bytes / xcs_row_bytes(sh));
  PAR_REQUIRE(Cp >= 1, PAR_ERR_WORKSPACE, "par_find_delay_sect_f64: scratch holds less than one row (%zu bytes)", xcs_row_bytes(sh));
  if (Cp > kXcbMaxPass) Cp = kXcbMaxPass;
  if (Cp > n_win) Cp = n_win;
  PAR_HIP_CHECK(hipSetDevice(device));
  hipStream_t s = as_stream(stream);
  const int64_t N = sh.N, DN = (int64_t)sh.D * N;
  float2* X = static_cast<float2*>(scratch);        // z_s, then the diagonals C_d
  float2* Y = X + Cp * DN;                          // the section spectra, then the diagonals' lags
  XcbRow* rows = reinterpret_cast<XcbRow*>(Y + Cp * DN);
  for (int64_t w0 = 0; w0 < n_win; w0 += Cp) {
    const int64_t c = n_win - w0 < Cp ? n_win - w0 : Cp;
    const double* ac = a + w0 * a_pitch;
    const double* bc = b + w0 * b_pitch;
    hipLaunchKernelGGL(k_xcb_norms, dim3(2, (unsigned)c), dim3(1024), 0, s, ac, a_pitch, na, bc, b_pitch, nb, rows);
    hipLaunchKernelGGL(k_xcs_pack, dim3((unsigned)ceil_div(N, 256), (unsigned)sh.M, (unsigned)c), dim3(256), 0, s, ac, a_pitch, na, bc,
                       b_pitch, nb, (const XcbRow*)rows, X, sh.S, (int64_t)sh.M);
    int rc = big_fft_c2c(device, X, Y, N, c * sh.M, s);                 // Y = FFT(a_s + i b_s), section by section
    if (rc != PAR_OK) return rc;
    hipLaunchKernelGGL(k_xcs_diag, dim3((unsigned)ceil_div(N / 2 + 1, 256), (unsigned)sh.D, (unsigned)c), dim3(256), 0, s,
                       (const float2*)Y, X, N, sh.P, sh.Q);
    rc = big_fft_c2c(device, X, Y, N, c * sh.D, s);                     // Y = conj(N * circular correlation), diagonal by diagonal
    if (rc != PAR_OK) return rc;
    const XcLagsOfSect lags{Y, sh.S, sh.P, sh.Q};
    if (same_out)
      hipLaunchKernelGGL(k_xcs_same, dim3((unsigned)ceil_div(na, 256), (unsigned)c), dim3(256), 0, s, lags, na, nb,
                         same_out + w0 * same_pitch, same_pitch);
    if (norms)
      hipLaunchKernelGGL(k_xcs_norms_out, dim3((unsigned)ceil_div(c, 64)), dim3(64), 0, s, (const XcbRow*)rows, c, norms + 2 * w0);
    xc_search<XcLagsOfSect, 1024>(lags, ac, a_pitch, na, bc, b_pitch, nb, c, ignore_phase, rows, delay + w0, corr + w0, status + w0, s);
    PAR_HIP_CHECK(hipGetLastError());
  }
  return PAR_OK;
}

// Spectrum.get_signal (util/spectrum.py:158-171) for n_win windows of one channel: see include/par_hip.h.  The geometry is
// checked on the host, from the caller's host copy, before anything is launched.
int par_gather_windows_f64(int device, const float* sig, int64_t sig_stride, int64_t n, const int64_t* starts, const int64_t* lens,
                           const int64_t* pad_l, const int64_t* host_geom, int64_t n_win, int64_t n_out, double* out,
                           int64_t out_pitch, void* stream) {
  using namespace par;
  PAR_REQUIRE(sig && starts && lens && pad_l && host_geom && out, PAR_ERR_ARG, "par_gather_windows_f64: null pointer");
  PAR_REQUIRE(sig_stride >= 1 && n >= 0 && n_win >= 0 && n_out >= 0 && out_pitch >= n_out, PAR_ERR_ARG,
              "par_gather_windows_f64: stride %lld, n %lld, n_win %lld, n_out %lld, pitch %lld", (long long)sig_stride, (long long)n,
              (long long)n_win, (long long)n_out, (long long)out_pitch);
  for (int64_t w = 0; w < n_win; ++w) {
    const int64_t st = host_geom[w], ln = host_geom[n_win + w], pl = host_geom[2 * n_win + w];
    PAR_REQUIRE(st >= 0 && ln >= 0 && pl >= 0 && st <= n && ln <= n - st && pl <= n_out && ln <= n_out - pl, PAR_ERR_ARG,
                "par_gather_windows_f64: window %lld (start %lld, length %lld, pad %lld) leaves the %lld-sample signal or the %lld-sample row",
                (long long)w, (long long)st, (long long)ln, (long long)pl, (long long)n, (long long)n_out);
  }
  if (n_win == 0 || n_out == 0) return PAR_OK;
  PAR_HIP_CHECK(hipSetDevice(device));
  for (int64_t w0 = 0; w0 < n_win; w0 += kXcbMaxPass) {
    const int64_t c = n_win - w0 < kXcbMaxPass ? n_win - w0 : kXcbMaxPass;
    hipLaunchKernelGGL(k_gather_windows, dim3((unsigned)ceil_div(n_out, 256), (unsigned)c), dim3(256), 0, as_stream(stream), sig,
                       sig_stride, n, reinterpret_cast<const long long*>(starts), reinterpret_cast<const long long*>(lens),
                       reinterpret_cast<const long long*>(pad_l), w0, n_out, out, out_pitch);
  }
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}

int par_istft_f32(int device, const float* spec, int64_t n_frames, int n_fft, int hop, const float* window,
                  float* frames, float* y, int64_t y_len, int64_t skip, void* stream) {
  using namespace par;
  PAR_REQUIRE(spec && window && y, PAR_ERR_ARG, "par_istft_f32: null pointer");
  PAR_REQUIRE(n_frames >= 1 && hop >= 1 && y_len >= 0 && skip >= 0, PAR_ERR_ARG, "par_istft_f32: bad sizes");
  PAR_REQUIRE(n_fft >= 16 && n_fft <= (1 << 21) && (n_fft & (n_fft - 1)) == 0, PAR_ERR_UNSUPPORTED,
              "par_istft_f32: n_fft=%d is not a power of two in [16, 2^21]", n_fft);
  // (before any HIP call, like the other argument errors: a caller without the scratch hears so on any machine)
  PAR_REQUIRE(frames || (n_fft <= 8192 && istft_is_fused(n_fft, hop)), PAR_ERR_ARG,
              "par_istft_f32: n_fft=%d hop=%d needs the frames scratch (par_istft_scratch_floats)", n_fft, hop);
  PAR_HIP_CHECK(hipSetDevice(device));
  if (n_fft > 8192) {                              // frames of the four-step size class (the GUI's FFT sizes go to 2^20)
    const int64_t H = n_fft / 2, B = istft_big_batch(n_frames, n_fft);
    float2* A = reinterpret_cast<float2*>(frames + ((n_frames * (int64_t)n_fft + 3) & ~3ll));
    float2* V = A + B * H;
    const float scale = (float)(sqrt((double)n_fft) / (double)H);
    for (int64_t f0 = 0; f0 < n_frames; f0 += B) {
      const int64_t nb = n_frames - f0 < B ? n_frames - f0 : B;
      hipLaunchKernelGGL(k_ibig_pack, dim3((unsigned)ceil_div(nb * H, 256)), dim3(256), 0, as_stream(stream),
                         reinterpret_cast<const float2*>(spec), f0, nb, H, A);
      int rc2 = big_fft_c2c(device, A, V, H, nb, as_stream(stream));
      if (rc2 != PAR_OK) return rc2;
      hipLaunchKernelGGL(k_ibig_unpack, dim3((unsigned)ceil_div(nb * H, 256)), dim3(256), 0, as_stream(stream), (const float2*)V,
                         f0, nb, H, window, frames, scale);
    }
    PAR_HIP_CHECK(hipGetLastError());
    if (y_len > 0) {
      hipLaunchKernelGGL(k_istft_ola, dim3((unsigned)ceil_div(y_len, 256)), dim3(256), 0, as_stream(stream), frames, n_frames,
                         n_fft, hop, window, y, y_len, skip);
      PAR_HIP_CHECK(hipGetLastError());
    }
    return PAR_OK;
  }
  Twiddles tw;
  int rc = get_twiddles(device, n_fft, &tw);
  if (rc != PAR_OK) return rc;
  const int H = n_fft / 2;
  // spec * sqrt(n_fft) (:359) and the 1/H of the H-point complex inverse fold into one factor
  const float scale = (float)(sqrt((double)n_fft) / (double)H);
  const float2* sp2 = reinterpret_cast<const float2*>(spec);
  if (istft_is_fused(n_fft, hop)) {
    if (y_len == 0) return PAR_OK;
    const int s = (n_fft + hop - 1) / hop;
    return dispatch_logh<3, 12>(ilog2(H), [&](auto lh) {
      constexpr int LH = decltype(lh)::value;
      const int64_t out_len = (int64_t)(FftGeom<LH>::Frames * s - s + 1) * hop;
      return launch_with_lds(k_istft_fused<LH>, dim3((unsigned)ceil_div(y_len + skip, out_len)), dim3(FftGeom<LH>::Threads),
                             istft_fused_lds<LH>(hop), device, as_stream(stream), sp2, n_frames, hop, s, window, tw.w, tw.post, y, y_len,
                             skip, scale);
    });
  }
  rc = dispatch_logh<3, 12>(ilog2(H), [&](auto lh) {
    using G = FftGeom<decltype(lh)::value>;
    return launch_with_lds(k_istft_frames<decltype(lh)::value>, dim3((unsigned)ceil_div(n_frames, G::Frames)), dim3(G::Threads), G::FramesLds,
                           device, as_stream(stream), sp2, n_frames, window, tw.w, tw.post, frames, scale);
  });
  if (rc != PAR_OK) return rc;
  if (y_len > 0) {
    hipLaunchKernelGGL(k_istft_ola, dim3((unsigned)ceil_div(y_len, 256)), dim3(256), 0, as_stream(stream), frames,
                       n_frames, n_fft, hop, window, y, y_len, skip);
    PAR_HIP_CHECK(hipGetLastError());
  }
  return PAR_OK;
}

}  // extern "C"

// ---- spectral gain mask (config 4, dropout_healer_gui.py:161-162): S *= 10^(gain_db/20) ----------------
namespace par {
__global__ void k_apply_gain_db(float2* __restrict__ spec, const float* __restrict__ gain_db, int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const float g = gain_db[i];
  if (g == 0.0f) return;                               // np.power(10, 0/20) == 1 exactly
  const float f = exp2f(g * 0.16609640474436813f);     // 10^(g/20) = 2^(g*log2(10)/20)
  float2 v = spec[i];
  v.x *= f;
  v.y *= f;
  spec[i] = v;
}
}  // namespace par

extern "C" int par_spec_apply_gain_db_c64(int device, float* spec, const float* gain_db, int64_t count, void* stream) {
  using namespace par;
  PAR_REQUIRE(spec && gain_db && count >= 0, PAR_ERR_ARG, "par_spec_apply_gain_db_c64: bad args");
  if (count == 0) return PAR_OK;
  PAR_HIP_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_apply_gain_db, dim3((unsigned)ceil_div(count, 256)), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<float2*>(spec), gain_db, count);
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}

// ---- renoiser gate entry points (ABI 108) -------------------------------------------------------------------------------------
extern "C" int par_gate_spectrum_f32(int device, float* spec, int64_t n_frames, int64_t bins, int64_t pitch, const float* cutoff,
                                     float low, void* stream) {
  using namespace par;
  PAR_REQUIRE(spec && cutoff, PAR_ERR_ARG, "par_gate_spectrum_f32: null pointer");
  const int64_t p = pitch ? pitch : bins;
  PAR_REQUIRE(n_frames >= 0 && bins >= 1 && p >= bins, PAR_ERR_ARG, "par_gate_spectrum_f32: bad sizes (frames %lld, bins %lld, pitch %lld)",
              (long long)n_frames, (long long)bins, (long long)pitch);
  PAR_REQUIRE(ceil_div(bins, 256) <= 0x7fffffff, PAR_ERR_UNSUPPORTED, "par_gate_spectrum_f32: too many bins");
  if (n_frames == 0) return PAR_OK;
  PAR_HIP_CHECK(hipSetDevice(device));
  const int64_t gy = n_frames < 4096 ? n_frames : 4096;
  hipLaunchKernelGGL(k_gate_spectrum, dim3((unsigned)ceil_div(bins, 256), (unsigned)gy), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<float2*>(spec), n_frames, bins, p, cutoff, low);
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}

static int gate_stft_sizes(int64_t n, int n_fft, int hop, int64_t* n_frames_i, int* s, int* rounds, int* ring, int64_t* runs,
                           size_t* lds, int* frames_per_round) {
  using namespace par;
  if (n < 1 || hop < 1 || hop > n_fft || n_fft < 16 || n_fft > 8192 || (n_fft & (n_fft - 1))) return PAR_ERR_UNSUPPORTED;
  const int64_t frames = par_stft_frames(n + n_fft / 2, n_fft, hop);                    // STFT of fix_length(x, n + n_fft/2)
  const int64_t want = ceil_div(n + n_fft, hop);                                        // istft(length=n) keeps these
  *n_frames_i = frames < want ? frames : want;
  *s = (int)ceil_div(n_fft, hop);
  return dispatch_logh<3, 12>(ilog2(n_fft / 2), [&](auto lh) {
    using GG = GateGeom<decltype(lh)::value>;
    *frames_per_round = GG::G::Frames;
    *rounds = GG::rounds(*s);
    *ring = GG::ring(hop);
    *lds = GG::lds(hop);
    *runs = ceil_div(n + n_fft / 2, (int64_t)(GG::G::Frames * *rounds - (*s - 1)) * hop);
    return (*lds <= 160 * 1024) ? PAR_OK : PAR_ERR_UNSUPPORTED;
  });
}

extern "C" int64_t par_gate_stft_transformed_frames(int64_t n, int n_fft, int hop) {
  int64_t nfi = 0, runs = 0;
  int s = 0, rounds = 0, ring = 0, frames_per_round = 0;
  size_t lds = 0;
  if (gate_stft_sizes(n, n_fft, hop, &nfi, &s, &rounds, &ring, &runs, &lds, &frames_per_round) != PAR_OK) return 0;
  // every run but the last transforms all its rounds; the last stops once its rounds reach the end of the output
  const int64_t out = (int64_t)frames_per_round * rounds - (s - 1);
  int64_t total = 0;
  for (int64_t b = 0; b < runs; ++b) {
    const int64_t f_start = b * out - (s - 1), st_hi = (b + 1) * out * hop < n + n_fft / 2 ? (b + 1) * out * hop : n + n_fft / 2;
    for (int r = 0; r < rounds; ++r) {
      if ((f_start + (int64_t)r * frames_per_round) * hop >= st_hi) break;
      total += frames_per_round;
    }
  }
  return total;
}

extern "C" int par_gate_stft_f32(int device, const float* x, int64_t n, int64_t x_stride, int n_ch, int n_fft, int hop,
                                 const float* window, const float* cutoff, float low, float* y, int64_t y_stride, void* stream) {
  using namespace par;
  PAR_REQUIRE(x && window && cutoff && y, PAR_ERR_ARG, "par_gate_stft_f32: null pointer");
  PAR_REQUIRE(n >= 1 && n_ch >= 1 && n_ch <= 65535 && x_stride >= n_ch && y_stride >= n_ch && hop >= 1, PAR_ERR_ARG,
              "par_gate_stft_f32: bad sizes (n %lld, channels %d, strides %lld / %lld, hop %d)", (long long)n, n_ch,
              (long long)x_stride, (long long)y_stride, hop);
  int64_t nfi = 0, runs = 0;
  int s = 0, rounds = 0, ring = 0, frames_per_round = 0;
  size_t lds = 0;
  PAR_REQUIRE(gate_stft_sizes(n, n_fft, hop, &nfi, &s, &rounds, &ring, &runs, &lds, &frames_per_round) == PAR_OK, PAR_ERR_UNSUPPORTED,
              "par_gate_stft_f32: n_fft=%d hop=%d (a power of two in [16, 8192], 1 <= hop <= n_fft)", n_fft, hop);
  PAR_REQUIRE(runs <= 0x7fffffff, PAR_ERR_UNSUPPORTED, "par_gate_stft_f32: signal too long");
  PAR_HIP_CHECK(hipSetDevice(device));
  Twiddles tw;
  int rc = get_twiddles(device, n_fft, &tw);
  if (rc != PAR_OK) return rc;
  const float fscale = (float)(1.0 / sqrt((double)n_fft));
  const float iscale = (float)(sqrt((double)n_fft) / (double)(n_fft / 2));
  return dispatch_logh<3, 12>(ilog2(n_fft / 2), [&](auto lh) {
    return launch_with_lds(k_gate_stft<decltype(lh)::value>, dim3((unsigned)runs, (unsigned)n_ch), dim3(FftGeom<decltype(lh)::value>::Threads),
                           lds, device, as_stream(stream), x, n, x_stride, hop, s, rounds, ring, window, tw.w, tw.post, cutoff, low, y,
                           y_stride, nfi, fscale, iscale);
  });
}

// ---- MaxMono entry points (added at ABI 109) -----------------------------------------------------------------------------------
static bool ranges_overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return a && b && pa < pb + bytes && pb < pa + bytes;
}

extern "C" int par_select_spectrum_f32(int device, const float* specL, const float* specR, int64_t n_frames, int64_t bins, int64_t pitch,
                                       float* out_max, float* out_min, void* stream) {
  using namespace par;
  PAR_REQUIRE(specL && specR && (out_max || out_min), PAR_ERR_ARG, "par_select_spectrum_f32: null pointer");
  const int64_t p = pitch ? pitch : bins;
  PAR_REQUIRE(n_frames >= 0 && bins >= 1 && p >= bins, PAR_ERR_ARG, "par_select_spectrum_f32: bad sizes (frames %lld, bins %lld, pitch %lld)",
              (long long)n_frames, (long long)bins, (long long)pitch);
  PAR_REQUIRE(ceil_div(bins, 256) <= 0x7fffffff, PAR_ERR_UNSUPPORTED, "par_select_spectrum_f32: too many bins");
  if (n_frames == 0) return PAR_OK;
  const size_t bytes = (size_t)((n_frames - 1) * p + bins) * sizeof(float2);
  PAR_REQUIRE(!ranges_overlap(out_max, specL, bytes) && !ranges_overlap(out_max, specR, bytes) && !ranges_overlap(out_min, specL, bytes) &&
                  !ranges_overlap(out_min, specR, bytes) && !ranges_overlap(out_max, out_min, bytes),
              PAR_ERR_ARG, "par_select_spectrum_f32: an output overlaps an input or the other output");
  PAR_HIP_CHECK(hipSetDevice(device));
  const int64_t gy = n_frames < 4096 ? n_frames : 4096;
  hipLaunchKernelGGL(k_select_spectrum, dim3((unsigned)ceil_div(bins, 256), (unsigned)gy), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const float2*>(specL), reinterpret_cast<const float2*>(specR), n_frames, bins, p,
                     reinterpret_cast<float2*>(out_max), reinterpret_cast<float2*>(out_min));
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}

static int maxmono_stft_sizes(int64_t n, int n_fft, int hop, int64_t* n_frames_i, int* s, int* rounds, int* ring, int64_t* runs,
                              size_t* lds, int* frames_per_round) {
  using namespace par;
  if (n < 1 || hop < 1 || hop > n_fft || n_fft < 16 || n_fft > 8192 || (n_fft & (n_fft - 1))) return PAR_ERR_UNSUPPORTED;
  const int64_t frames = par_stft_frames(n + n_fft / 2, n_fft, hop);                    // STFT of fix_length(x, n + n_fft/2)
  const int64_t want = ceil_div(n + n_fft, hop);                                        // istft(length=n) keeps these
  *n_frames_i = frames < want ? frames : want;
  *s = (int)ceil_div(n_fft, hop);
  return dispatch_logh<3, 12>(ilog2(n_fft / 2), [&](auto lh) {
    using MG = MaxMonoGeom<decltype(lh)::value>;
    *frames_per_round = MG::G::Frames;
    *rounds = MG::rounds(*s);
    *ring = MG::ring(hop);
    *lds = MG::lds(hop);
    *runs = ceil_div(n + n_fft / 2, (int64_t)(MG::G::Frames * *rounds - (*s - 1)) * hop);
    return (*lds <= 160 * 1024) ? PAR_OK : PAR_ERR_UNSUPPORTED;
  });
}

extern "C" int par_maxmono_stft_supported(int n_fft, int hop) {
  int64_t nfi = 0, runs = 0;
  int s = 0, rounds = 0, ring = 0, frames_per_round = 0;
  size_t lds = 0;
  return maxmono_stft_sizes(1, n_fft, hop, &nfi, &s, &rounds, &ring, &runs, &lds, &frames_per_round) == PAR_OK;
}

extern "C" int64_t par_maxmono_stft_transformed_frames(int64_t n, int n_fft, int hop) {
  int64_t nfi = 0, runs = 0;
  int s = 0, rounds = 0, ring = 0, frames_per_round = 0;
  size_t lds = 0;
  if (maxmono_stft_sizes(n, n_fft, hop, &nfi, &s, &rounds, &ring, &runs, &lds, &frames_per_round) != PAR_OK) return 0;
  // every run but the last transforms all its rounds; the last stops once its rounds reach the end of the output
  const int64_t out = (int64_t)frames_per_round * rounds - (s - 1);
  int64_t total = 0;
  for (int64_t b = 0; b < runs; ++b) {
    const int64_t f_start = b * out - (s - 1), st_hi = (b + 1) * out * hop < n + n_fft / 2 ? (b + 1) * out * hop : n + n_fft / 2;
    for (int r = 0; r < rounds; ++r) {
      if ((f_start + (int64_t)r * frames_per_round) * hop >= st_hi) break;
      total += frames_per_round;
    }
  }
  return total;
}

extern "C" int par_maxmono_stft_f32(int device, const float* xL, const float* xR, int64_t n, int64_t x_stride, int n_fft, int hop,
                                    const float* window, float* y_max, int64_t ymax_stride, float* y_min, int64_t ymin_stride,
                                    void* stream) {
  using namespace par;
  PAR_REQUIRE(xL && xR && window && (y_max || y_min), PAR_ERR_ARG, "par_maxmono_stft_f32: null pointer");
  PAR_REQUIRE(n >= 1 && x_stride >= 1 && (!y_max || ymax_stride >= 1) && (!y_min || ymin_stride >= 1) && hop >= 1, PAR_ERR_ARG,
              "par_maxmono_stft_f32: bad sizes (n %lld, strides %lld / %lld / %lld, hop %d)", (long long)n, (long long)x_stride,
              (long long)ymax_stride, (long long)ymin_stride, hop);
  int64_t nfi = 0, runs = 0;
  int s = 0, rounds = 0, ring = 0, frames_per_round = 0;
  size_t lds = 0;
  PAR_REQUIRE(maxmono_stft_sizes(n, n_fft, hop, &nfi, &s, &rounds, &ring, &runs, &lds, &frames_per_round) == PAR_OK, PAR_ERR_UNSUPPORTED,
              "par_maxmono_stft_f32: n_fft=%d hop=%d (a power of two in [16, 8192], 1 <= hop <= n_fft, two rings within 160 KB of LDS)",
              n_fft, hop);
  PAR_REQUIRE(runs <= 0x7fffffff, PAR_ERR_UNSUPPORTED, "par_maxmono_stft_f32: signal too long");
  PAR_HIP_CHECK(hipSetDevice(device));
  Twiddles tw;
  int rc = get_twiddles(device, n_fft, &tw);
  if (rc != PAR_OK) return rc;
  const float fscale = (float)(1.0 / sqrt((double)n_fft));
  const float iscale = (float)(sqrt((double)n_fft) / (double)(n_fft / 2));
  return dispatch_logh<3, 12>(ilog2(n_fft / 2), [&](auto lh) {
    return launch_with_lds(k_maxmono_stft<decltype(lh)::value>, dim3((unsigned)runs), dim3(FftGeom<decltype(lh)::value>::Threads), lds,
                           device, as_stream(stream), xL, xR, n, x_stride, hop, s, rounds, ring, window, tw.w, tw.post, y_max,
                           ymax_stride, y_min, ymin_stride, nfi, fscale, iscale);
  });
}
