// K_gauge -- the renoiser's "Gauge offset" (renoiser_gui.py:347-369, prototype experiments/renoiser.py:59-73) without a
// spectrogram.  For every pad i < hop the reference puts i zeros in front of the channel, zero-extends it by n_fft/2, takes a
// complex STFT (reflect padding n_fft/2), averages bins l..u-1 of every frame and takes the standard deviation of that complex
// series over the frames.  The mean of bins l..u-1 of a windowed frame is the inner product of the frame with one complex
// vector h (renoiser.gauge_filter), so every (pad, frame) value is one tap sum
//     z(i, j) = sum_m p_i[j hop + m] h[m],      m = 0 .. n_fft - 1 ascending, float32, one FMA per tap and part,
// over the padded signal p_i.  With half = n_fft / 2 and M = n + i + half, padded index q maps to r = q - half; r < 0 reflects
// to -r, r >= M to 2 (M - 1) - r; the value is x[r - i] for i <= r < i + n and 0 elsewhere.  The padded signal has M + 2 half
// samples and so (M + 2 half - n_fft) / hop + 1 frames (ga_frames): no frame reads past it, also for an odd n_fft.
//
// A frame whose window touches no reflected sample starts at signal position t = j hop - half - i and reads the zero-extended
// signal xe[t .. t + n_fft): for 0 <= t <= n + half - n_fft every t belongs to exactly one (i, j), i = (-(t + half)) mod hop.
// So the interior is one n_fft-tap complex FIR evaluated at every t ("dense"), sorted into hop residue classes; all other
// frames ("edge", at most a few n_fft / hop per pad) go through the index map above.
//
// Two launches:
//   k_gauge_taps   all tap sums.
//     dense workgroups: kGaTile consecutive t each, a lane 8 consecutive t.  The taps are walked in chunks of kGaChunk (any
//                  n_fft: the chunk loop, not LDS, bounds the filter); per chunk the signal tile + halo is staged in LDS (zero
//                  outside [0, n)), a lane reads its 24-sample window of a 16-tap block with six ds_read_b128 and spends 256
//                  FMAs on it; h[m] is wave-uniform, staged in LDS with the chunk and read as broadcasts into registers.  The tile's z are then summed per residue class, ascending
//                  t, in float64 (sum re, sum im, sum |z|^2, each a Neumaier sum) into partial[workgroup][slot].
//     edge workgroups (the first of the grid, so their gathers hide behind the dense ones): one lane per (pad, edge frame),
//                  the same ascending FMA chain over the index map, z to ez[e][pad].
//   k_gauge_final  one workgroup per pad: lane th sums the partials of its contiguous run of dense workgroups (ascending) and
//                  the edge values e = th, th + 256, .. (Neumaier sums), a fixed 256-leaf tree joins the lanes;
//                  std = sqrt(max(0, S2 / F - |S / F|^2)) (numpy's std of a complex array, ddof 0).
// No atomics: two runs are bit-identical.
#include "par_common.h"
#include <math.h>

namespace par {

constexpr int kGaBlock = 256;
constexpr int kGaPer = 8;                          // consecutive outputs per lane
constexpr int kGaTile = kGaBlock * kGaPer;         // 2048 outputs per workgroup
constexpr int kGaChunk = 1024;                     // taps per staged chunk
constexpr int kGaTapBlock = 16;                    // taps per register window
constexpr int kGaStage = kGaTile + kGaChunk + 16;  // staged samples: the last lane's window of the last block ends at + 8
constexpr int kGaLds = kGaStage + 2 * kGaChunk;    // floats: signal, then the chunk's h_re and h_im; reused for the tile's z
static_assert(kGaLds >= 2 * kGaTile, "the tile's z (float2) reuse the staging buffer");

struct GaGeom {
  int64_t n, xs;
  int n_fft, hop, half;
  int ext;                // half - (n_fft odd): the last frame starts at or before n + i + ext (ga_frames)
  int64_t dense;          // dense positions t = 0 .. dense - 1 (0: none)
  int64_t n_wg;           // dense workgroups
  int slots;              // residue slots per workgroup: min(hop, kGaTile)
  int edges;              // edge frames per pad, at most
  int edge_blocks;        // workgroups that take the edges hop edge lanes
};

// frames of the signal of M = n + i + half samples reflect-padded by half at both ends: (M + 2 half - n_fft) / hop + 1, which is
// (n + i + half) / hop + 1 for an even n_fft and one frame fewer where hop divides M for an odd one.  ext = 3 half - n_fft (GaGeom)
__host__ __device__ inline int ga_ext(int n_fft) { return n_fft / 2 - (n_fft & 1); }
__host__ __device__ inline int64_t ga_frames(int64_t n, int ext, int hop, int i) { return (n + i + ext) / hop + 1; }
// dense frames of pad i: j_lo .. j_hi (inclusive; empty when j_lo > j_hi)
__host__ __device__ inline int64_t ga_j_lo(const GaGeom& g, int i) { return ((int64_t)g.half + i + g.hop - 1) / g.hop; }
__host__ __device__ inline int64_t ga_j_hi(const GaGeom& g, int i) {
  return g.dense > 0 ? (g.dense - 1 + g.half + i) / g.hop : -1;
}

// Neumaier's compensated sum: s + c is the running total
__device__ __forceinline__ void ga_add(double& s, double& c, double v) {
  const double t = s + v;
  c += fabs(s) >= fabs(v) ? (s - t) + v : (v - t) + s;
  s = t;
}

// dense workgroup wg: z of t = wg kGaTile .. + kGaTile, summed per residue class into partial[wg][slot]
__device__ __forceinline__ void ga_dense(const float* __restrict__ x, const float* __restrict__ h_re,
                                         const float* __restrict__ h_im, const GaGeom& g, double* __restrict__ partial,
                                         int64_t wg, float* lds) {
  const int tid = threadIdx.x;
  const int64_t base = wg * kGaTile;
  float are[kGaPer], aim[kGaPer];
#pragma unroll
  for (int r = 0; r < kGaPer; ++r) are[r] = aim[r] = 0.0f;
  for (int c0 = 0; c0 < g.n_fft; c0 += kGaChunk) {
    const int kc = g.n_fft - c0 < kGaChunk ? g.n_fft - c0 : kGaChunk;
    __syncthreads();                                  // the previous chunk's reads are done
    for (int k = tid; k < kGaStage; k += kGaBlock) {
      const int64_t s = base + c0 + k;
      lds[k] = s < g.n ? x[s * g.xs] : 0.0f;
    }
    float* hs_re = lds + kGaStage;
    float* hs_im = hs_re + kGaChunk;
    for (int k = tid; k < kc; k += kGaBlock) hs_re[k] = h_re[c0 + k], hs_im[k] = h_im[c0 + k];
    __syncthreads();
    const float* win = lds + tid * kGaPer;
    int m0 = 0;
    for (; m0 + kGaTapBlock <= kc; m0 += kGaTapBlock) {
      float w[kGaTapBlock + kGaPer];
#pragma unroll
      for (int v = 0; v < (kGaTapBlock + kGaPer) / 4; ++v) {
        const float4 f = *reinterpret_cast<const float4*>(win + m0 + 4 * v);
        w[4 * v] = f.x, w[4 * v + 1] = f.y, w[4 * v + 2] = f.z, w[4 * v + 3] = f.w;
      }
      // the taps come from LDS too (one address for the whole wave: a broadcast read): v_fma_f32 with three vector operands
      // issues every 2.8 cycles per SIMD here, with a scalar operand every 4.6 (profiles/r02_ubench2_gfx950.txt)
      float hr[kGaTapBlock], hi[kGaTapBlock];
#pragma unroll
      for (int v = 0; v < kGaTapBlock / 4; ++v) {
        const float4 a = *reinterpret_cast<const float4*>(hs_re + m0 + 4 * v);
        const float4 b = *reinterpret_cast<const float4*>(hs_im + m0 + 4 * v);
        hr[4 * v] = a.x, hr[4 * v + 1] = a.y, hr[4 * v + 2] = a.z, hr[4 * v + 3] = a.w;
        hi[4 * v] = b.x, hi[4 * v + 1] = b.y, hi[4 * v + 2] = b.z, hi[4 * v + 3] = b.w;
      }
#pragma unroll
      for (int k = 0; k < kGaTapBlock; ++k) {
#pragma unroll
        for (int r = 0; r < kGaPer; ++r) {
          are[r] = fmaf(w[k + r], hr[k], are[r]);
          aim[r] = fmaf(w[k + r], hi[k], aim[r]);
        }
      }
    }
    for (; m0 < kc; ++m0) {                           // the last taps of an n_fft that is no multiple of 16
      const float cr = hs_re[m0], ci = hs_im[m0];
#pragma unroll
      for (int r = 0; r < kGaPer; ++r) {
        const float v = win[m0 + r];
        are[r] = fmaf(v, cr, are[r]);
        aim[r] = fmaf(v, ci, aim[r]);
      }
    }
  }
  __syncthreads();
  float2* zs = reinterpret_cast<float2*>(lds);
#pragma unroll
  for (int r = 0; r < kGaPer; ++r) zs[tid * kGaPer + r] = make_float2(are[r], aim[r]);
  __syncthreads();
  const int64_t left = g.dense - base;
  const int valid = left < kGaTile ? (int)left : kGaTile;
  for (int s = tid; s < g.slots; s += kGaBlock) {
    double sr = 0.0, cr = 0.0, si = 0.0, ci = 0.0, sq = 0.0, cq = 0.0;
    for (int k = s; k < valid; k += g.hop) {
      const double a = (double)zs[k].x, b = (double)zs[k].y;
      ga_add(sr, cr, a);
      ga_add(si, ci, b);
      ga_add(sq, cq, a * a + b * b);
    }
    double* p = partial + (wg * g.slots + s) * 3;
    p[0] = sr + cr, p[1] = si + ci, p[2] = sq + cq;
  }
}

// edge frame e of pad i -> frame number (a frame past the last one: -1)
__device__ __forceinline__ int64_t ga_edge_frame(const GaGeom& g, int i, int e) {
  const int64_t j_lo = ga_j_lo(g, i), j_hi = ga_j_hi(g, i), frames = ga_frames(g.n, g.ext, g.hop, i);
  int64_t j;
  if (j_lo > j_hi) j = e;                             // no dense frame: every frame is an edge frame
  else j = e < j_lo ? e : j_hi + 1 + (e - j_lo);
  return j < frames ? j : -1;
}

// edge lane id = e hop + i: frame ga_edge_frame(i, e) of pad i through the index map, the same ascending chain; the loads of
// eight taps are issued together (they do not depend on the sums)
__device__ __forceinline__ void ga_edge(const float* __restrict__ x, const float* __restrict__ h_re,
                                        const float* __restrict__ h_im, const GaGeom& g, float2* __restrict__ ez, int64_t id) {
  if (id >= (int64_t)g.edges * g.hop) return;
  const int i = (int)(id % g.hop), e = (int)(id / g.hop);
  const int64_t j = ga_edge_frame(g, i, e);
  float re = 0.0f, im = 0.0f;
  if (j >= 0) {
    const int64_t M = g.n + i + g.half;
    const int64_t r0 = j * g.hop - g.half;
    for (int m0 = 0; m0 < g.n_fft; m0 += 8) {
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        int64_t r = r0 + m0 + k;
        if (r < 0) r = -r;
        else if (r >= M) r = 2 * (M - 1) - r;
        const int64_t s = r - i;
        v[k] = (m0 + k < g.n_fft && r >= 0 && r < M && s >= 0 && s < g.n) ? x[s * g.xs] : 0.0f;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (m0 + k < g.n_fft) {
          re = fmaf(v[k], h_re[m0 + k], re);
          im = fmaf(v[k], h_im[m0 + k], im);
        }
    }
  }
  ez[id] = make_float2(re, im);
}

// one launch for all tap sums: the first g.edge_blocks workgroups take the edge frames (latency-bound gathers, hidden behind
// the dense workgroups that follow them)
__global__ __launch_bounds__(kGaBlock) void k_gauge_taps(const float* __restrict__ x, const float* __restrict__ h_re,
                                                         const float* __restrict__ h_im, GaGeom g, double* __restrict__ partial,
                                                         float2* __restrict__ ez) {
  __shared__ __attribute__((aligned(16))) float lds[kGaLds];
  if ((int)blockIdx.x < g.edge_blocks) ga_edge(x, h_re, h_im, g, ez, (int64_t)blockIdx.x * kGaBlock + threadIdx.x);
  else ga_dense(x, h_re, h_im, g, partial, (int64_t)blockIdx.x - g.edge_blocks, lds);
}

__global__ __launch_bounds__(kGaBlock) void k_gauge_final(const double* __restrict__ partial, const float2* __restrict__ ez,
                                                          GaGeom g, double* __restrict__ stds) {
  __shared__ double red[3][kGaBlock];
  const int i = blockIdx.x, th = threadIdx.x;
  double sr = 0.0, cr = 0.0, si = 0.0, ci = 0.0, sq = 0.0, cq = 0.0;
  const int64_t per = (g.n_wg + kGaBlock - 1) / kGaBlock;
  const int64_t w_end = (th + 1) * per < g.n_wg ? (th + 1) * per : g.n_wg;
  // a dense t of pad i has t = -(half + i) mod hop; in workgroup w that is slot (t - w kGaTile) mod hop
  const int64_t res = ((-(int64_t)(g.half + i)) % g.hop + g.hop) % g.hop;
  for (int64_t w = th * per; w < w_end; ++w) {
    const int64_t c = ((res - (w * kGaTile) % g.hop) % g.hop + g.hop) % g.hop;
    if (c >= g.slots) continue;
    const double* p = partial + (w * g.slots + c) * 3;
    ga_add(sr, cr, p[0]);
    ga_add(si, ci, p[1]);
    ga_add(sq, cq, p[2]);
  }
  for (int e = th; e < g.edges; e += kGaBlock) {
    if (ga_edge_frame(g, i, e) < 0) continue;
    const float2 z = ez[(int64_t)e * g.hop + i];
    const double a = (double)z.x, b = (double)z.y;
    ga_add(sr, cr, a);
    ga_add(si, ci, b);
    ga_add(sq, cq, a * a + b * b);
  }
  red[0][th] = sr + cr, red[1][th] = si + ci, red[2][th] = sq + cq;
  __syncthreads();
  for (int s = kGaBlock / 2; s > 0; s >>= 1) {
    if (th < s) {
      red[0][th] += red[0][th + s];
      red[1][th] += red[1][th + s];
      red[2][th] += red[2][th + s];
    }
    __syncthreads();
  }
  if (th == 0) {
    const double F = (double)ga_frames(g.n, g.ext, g.hop, i);
    const double mr = red[0][0] / F, mi = red[1][0] / F;
    const double var = red[2][0] / F - (mr * mr + mi * mi);
    stds[i] = sqrt(var > 0.0 ? var : var == var ? 0.0 : var);      // the clamp keeps a NaN
  }
}

// false: the sizes do not fit the index arithmetic
static bool ga_geometry(int64_t n, int64_t xs, int n_fft, int hop, GaGeom* g) {
  if (n > (int64_t)1 << 46) return false;
  g->n = n, g->xs = xs, g->n_fft = n_fft, g->hop = hop, g->half = n_fft / 2, g->ext = ga_ext(n_fft);
  const int64_t dense = n + g->half - n_fft + 1;
  g->dense = dense > 0 ? dense : 0;
  g->n_wg = ceil_div(g->dense, kGaTile);
  g->slots = hop < kGaTile ? hop : kGaTile;
  // per pad: frames before the first dense one, j hop < half + i, and after the last, up to (n + i + ext) / hop --
  // or, with no dense frame at all, every frame (tests/gauge_inputs.py replays this count against ga_frames)
  int64_t edges;
  if (g->dense > 0) edges = ((int64_t)g->half + hop - 1) / hop + 1 + ((int64_t)n_fft - g->half) / hop + 2;
  else edges = (n + hop - 1 + g->half) / hop + 1;
  if (edges > (int64_t)1 << 24) return false;
  g->edges = (int)edges;
  const int64_t edge_blocks = ceil_div(edges * hop, kGaBlock);
  if (g->n_wg + edge_blocks > 0x7fffffff) return false;                                          // the grid
  g->edge_blocks = (int)edge_blocks;
  return true;
}

static size_t ga_partial_bytes(const GaGeom& g) { return (size_t)g.n_wg * g.slots * 3 * sizeof(double); }

}  // namespace par

extern "C" int64_t par_gauge_frames(int64_t n, int n_fft, int hop, int offset) {
  if (n < 0 || n_fft < 2 || hop < 1 || offset < 0) return -1;
  return par::ga_frames(n, par::ga_ext(n_fft), hop, offset);
}

extern "C" size_t par_gauge_scratch_bytes(int64_t n, int n_fft, int hop) {
  par::GaGeom g;
  if (n < 1 || n_fft < 2 || hop < 1 || !par::ga_geometry(n, 1, n_fft, hop, &g)) return 0;
  return par::ga_partial_bytes(g) + (size_t)g.edges * hop * sizeof(float2);
}

extern "C" int par_gauge_offset_f32(int device, const float* x, int64_t n, int64_t x_stride, int n_fft, int hop,
                                    const float* h_re, const float* h_im, double* stds, void* scratch, size_t scratch_bytes,
                                    void* stream) {
  using namespace par;
  PAR_REQUIRE(x, PAR_ERR_ARG, "par_gauge_offset_f32: null x");
  PAR_REQUIRE(h_re && h_im, PAR_ERR_ARG, "par_gauge_offset_f32: null h_re / h_im");
  PAR_REQUIRE(stds, PAR_ERR_ARG, "par_gauge_offset_f32: null stds");
  PAR_REQUIRE(n >= 1, PAR_ERR_ARG, "par_gauge_offset_f32: n %lld < 1", (long long)n);
  PAR_REQUIRE(n_fft >= 2, PAR_ERR_ARG, "par_gauge_offset_f32: n_fft %d < 2", n_fft);
  PAR_REQUIRE(hop >= 1, PAR_ERR_ARG, "par_gauge_offset_f32: hop %d < 1", hop);
  PAR_REQUIRE(x_stride >= 1, PAR_ERR_ARG, "par_gauge_offset_f32: x_stride %lld < 1", (long long)x_stride);
  GaGeom g;
  PAR_REQUIRE(ga_geometry(n, x_stride, n_fft, hop, &g), PAR_ERR_ARG, "par_gauge_offset_f32: n %lld with n_fft %d, hop %d is too long",
              (long long)n, n_fft, hop);
  const size_t need = par_gauge_scratch_bytes(n, n_fft, hop);
  PAR_REQUIRE(scratch, PAR_ERR_ARG, "par_gauge_offset_f32: null scratch");
  PAR_REQUIRE(scratch_bytes >= need, PAR_ERR_ARG, "par_gauge_offset_f32: scratch_bytes %zu, par_gauge_scratch_bytes gives %zu",
              scratch_bytes, need);
  PAR_REQUIRE(((uintptr_t)scratch & 7) == 0, PAR_ERR_ARG, "par_gauge_offset_f32: scratch is not 8-byte aligned");
  PAR_HIP_CHECK(hipSetDevice(device));
  hipStream_t s = as_stream(stream);
  double* partial = static_cast<double*>(scratch);
  float2* ez = reinterpret_cast<float2*>(static_cast<char*>(scratch) + ga_partial_bytes(g));
  hipLaunchKernelGGL(k_gauge_taps, dim3((unsigned)(g.edge_blocks + g.n_wg)), dim3(kGaBlock), 0, s, x, h_re, h_im, g, partial, ez);
  PAR_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_gauge_final, dim3((unsigned)hop), dim3(kGaBlock), 0, s, partial, ez, g, stds);
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}
