// K_pan -- the stereo balance tool (pypan_gui.py): the box measurement fac = np.nanmean(L[bL:bU, f0:f1] / R[bL:bU, f0:f1])
// of Canvas.on_mouse_release (:103) on magnitude spectrograms that exist, and the third np.interp call site,
// run_resample's signal[:, 1] * np.interp(arange(n), times * sr, pan) (:57-58).
//
// A measurement is split into work items, one per (box, frame): an item's lanes sum its cells' float32 quotients in
// float64 and count them, the item's pair goes to the caller's scratch, and k_pan_reduce folds a box's items in a fixed
// order.  No atomics anywhere, so two runs are bit-identical.  The fused form in stft.hip (k_stft_pan) produces the same
// items straight from the two channels and shares the scratch layout, the offsets and the reduction below:
//   scratch = int64 offs[n_box + 1] (padded to 16 bytes) | PanPart part[offs[n_box]]
// offs is the exclusive prefix sum of the boxes' item counts (pan_box_items), built on the device from the device copy of
// the boxes; the host computes the same numbers from its copy to size the scratch and the grids.
// Built with -ffp-contract=off (np_interp.h).
#include "pan_items.h"
#include "np_interp.h"
#include <math.h>

namespace par {

__global__ void k_pan_offsets(const int* __restrict__ boxes, int64_t n_box, int64_t* __restrict__ offs) {
  int64_t run = 0;
  for (int64_t b = 0; b < n_box; ++b) {
    offs[b] = run;
    run += pan_box_items(boxes + 4 * b);
  }
  offs[n_box] = run;
}

// One wave per item: the frame's row is contiguous in bins, so the 64 lanes read runs of 256 bytes of either channel.
constexpr int kPanCellWaves = 4;
__global__ __launch_bounds__(kPanCellWaves* kWave) void k_pan_cells(const float* __restrict__ magL, const float* __restrict__ magR,
                                                                     int64_t pitch, const int* __restrict__ boxes, int64_t n_box,
                                                                     const int64_t* __restrict__ offs, PanPart* __restrict__ part,
                                                                     int64_t n_items) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t item = (int64_t)blockIdx.x * kPanCellWaves + threadIdx.x / kWave;
  if (item >= n_items) return;                  // whole waves leave; nothing below synchronises the workgroup
  const int64_t box = pan_item_box(offs, n_box, item);
  const int* bx = boxes + 4 * box;
  const int64_t row = ((int64_t)bx[2] + (item - offs[box])) * pitch;
  double acc = 0.0;
  int cnt = 0;
  for (int b = bx[0] + lane; b < bx[1]; b += kWave) {
    const float q = __fdiv_rn(magL[row + b], magR[row + b]);          // numpy's float32 division, correctly rounded
    if (q == q) {                                                      // nanmean skips NaN cells; +-inf is summed
      acc += (double)q;
      ++cnt;
    }
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    acc += __shfl_xor(acc, o, kWave);
    cnt += __shfl_xor(cnt, o, kWave);
  }
  if (lane == 0) {
    part[item].sum = acc;
    part[item].cnt = cnt;
  }
}

// One workgroup per box: 256 strided runs over the box's items, ascending, then the xor tree and the four waves in order.
__global__ __launch_bounds__(256) void k_pan_reduce(const int64_t* __restrict__ offs, const PanPart* __restrict__ part,
                                                     double* __restrict__ fac, long long* __restrict__ count) {
  __shared__ double s_sum[256 / kWave];
  __shared__ long long s_cnt[256 / kWave];
  const int64_t box = blockIdx.x, lo = offs[box], hi = offs[box + 1];
  double acc = 0.0;
  long long cnt = 0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
    acc += part[i].sum;
    cnt += part[i].cnt;
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    acc += __shfl_xor(acc, o, kWave);
    cnt += __shfl_xor(cnt, o, kWave);
  }
  if ((threadIdx.x & (kWave - 1)) == 0) {
    s_sum[threadIdx.x / kWave] = acc;
    s_cnt[threadIdx.x / kWave] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    acc = s_sum[0];
    cnt = s_cnt[0];
    for (int w = 1; w < 256 / kWave; ++w) {
      acc += s_sum[w];
      cnt += s_cnt[w];
    }
    fac[box] = cnt ? acc / (double)cnt : __builtin_nan("");       // an empty slice or only NaN cells: nanmean gives NaN
    count[box] = cnt;
  }
}

// out = float32(float64(sig) * np.interp(i, xp, fp)): run_resample's product, stored as the FLOAT file stores it
__global__ __launch_bounds__(256) void k_pan_apply(const float* __restrict__ sig, int64_t sig_stride, int64_t n,
                                                    const double* __restrict__ xp, const double* __restrict__ fp, int64_t m,
                                                    float* __restrict__ out, int64_t out_stride) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  out[i * out_stride] = (float)((double)sig[i * sig_stride] * interp_one((double)i, xp, fp, m));
}

size_t pan_scratch_bytes(const int32_t* boxes_host, int64_t n_box) {
  if (!boxes_host || n_box < 1 || n_box > kPanMaxBoxes) return 0;
  int64_t items = 0;
  for (int64_t b = 0; b < n_box; ++b) items += pan_box_items(boxes_host + 4 * b);
  return pan_offs_bytes(n_box) + (size_t)items * sizeof(PanPart);
}

int pan_check_boxes(const char* who, const int32_t* boxes_host, int64_t n_box, int64_t bins, int64_t n_frames, int64_t* n_items) {
  int64_t items = 0;
  for (int64_t b = 0; b < n_box; ++b) {
    const int32_t* bx = boxes_host + 4 * b;
    // half-open ranges; an empty one (u <= l) is legal wherever its ends lie inside, as a numpy slice is
    PAR_REQUIRE(bx[0] >= 0 && bx[0] <= bins && bx[1] >= 0 && bx[1] <= bins && bx[2] >= 0 && bx[2] <= n_frames && bx[3] >= 0 &&
                    bx[3] <= n_frames,
                PAR_ERR_ARG, "%s: box %lld (bins [%d, %d), frames [%d, %d)) leaves the spectrogram of %lld bins x %lld frames", who,
                (long long)b, bx[0], bx[1], bx[2], bx[3], (long long)bins, (long long)n_frames);
    items += pan_box_items(bx);
  }
  PAR_REQUIRE(items <= 0x7fffffff, PAR_ERR_ARG, "%s: %lld (box, frame) items exceed one launch", who, (long long)items);
  *n_items = items;
  return PAR_OK;
}

void launch_pan_offsets(const int* boxes, int64_t n_box, void* scratch, hipStream_t s) {
  hipLaunchKernelGGL(k_pan_offsets, dim3(1), dim3(1), 0, s, boxes, n_box, reinterpret_cast<int64_t*>(scratch));
}

void launch_pan_reduce(int64_t n_box, const void* scratch, double* fac, int64_t* count, hipStream_t s) {
  hipLaunchKernelGGL(k_pan_reduce, dim3((unsigned)n_box), dim3(256), 0, s, reinterpret_cast<const int64_t*>(scratch),
                     reinterpret_cast<const PanPart*>(reinterpret_cast<const char*>(scratch) + pan_offs_bytes(n_box)), fac,
                     reinterpret_cast<long long*>(count));
}

}  // namespace par

extern "C" size_t par_pan_ratio_scratch_bytes(const int32_t* boxes_host, int64_t n_box) {
  return par::pan_scratch_bytes(boxes_host, n_box);
}

extern "C" int par_pan_ratio_f32(int device, const float* magL, const float* magR, int64_t n_frames, int64_t bins, int64_t pitch,
                                 const int32_t* boxes, const int32_t* boxes_host, int64_t n_box, double* fac, int64_t* count,
                                 void* scratch, size_t scratch_bytes, void* stream) {
  using namespace par;
  PAR_REQUIRE(magL && magR && boxes && boxes_host && fac && count && scratch, PAR_ERR_ARG, "par_pan_ratio_f32: null pointer");
  if (pitch == 0) pitch = bins;
  PAR_REQUIRE(n_frames >= 1 && bins >= 1 && bins <= 0x7fffffff && n_frames <= 0x7fffffff && pitch >= bins && n_box >= 1 &&
                  n_box <= kPanMaxBoxes,
              PAR_ERR_ARG, "par_pan_ratio_f32: bad sizes (n_frames %lld, bins %lld, pitch %lld, n_box %lld)", (long long)n_frames,
              (long long)bins, (long long)pitch, (long long)n_box);
  PAR_REQUIRE(((uintptr_t)scratch & 15) == 0, PAR_ERR_ARG, "par_pan_ratio_f32: scratch is not 16-byte aligned");
  int64_t n_items = 0;
  const int rc = pan_check_boxes("par_pan_ratio_f32", boxes_host, n_box, bins, n_frames, &n_items);
  if (rc != PAR_OK) return rc;
  PAR_REQUIRE(scratch_bytes >= pan_scratch_bytes(boxes_host, n_box), PAR_ERR_WORKSPACE, "par_pan_ratio_f32: scratch %zu < %zu",
              scratch_bytes, pan_scratch_bytes(boxes_host, n_box));
  PAR_HIP_CHECK(hipSetDevice(device));
  hipStream_t s = as_stream(stream);
  launch_pan_offsets(boxes, n_box, scratch, s);
  if (n_items > 0)
    hipLaunchKernelGGL(k_pan_cells, dim3((unsigned)ceil_div(n_items, kPanCellWaves)), dim3(kPanCellWaves * kWave), 0, s, magL, magR,
                       pitch, boxes, n_box, reinterpret_cast<const int64_t*>(scratch),
                       reinterpret_cast<PanPart*>(reinterpret_cast<char*>(scratch) + pan_offs_bytes(n_box)), n_items);
  launch_pan_reduce(n_box, scratch, fac, count, s);
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}

extern "C" int par_pan_apply_f32(int device, const float* sig, int64_t sig_stride, int64_t n, const double* xp, const double* fp,
                                 int64_t m, float* out, int64_t out_stride, void* stream) {
  using namespace par;
  PAR_REQUIRE(sig && xp && fp && out, PAR_ERR_ARG, "par_pan_apply_f32: null pointer");
  PAR_REQUIRE(m >= 1, PAR_ERR_ARG, "par_pan_apply_f32: need m >= 1 curve points (np.interp raises on an empty curve)");
  PAR_REQUIRE(n >= 0 && sig_stride >= 1 && out_stride >= 1, PAR_ERR_ARG, "par_pan_apply_f32: bad sizes");
  if (n == 0) return PAR_OK;
  PAR_HIP_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_pan_apply, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, as_stream(stream), sig, sig_stride, n, xp, fp, m,
                     out, out_stride);
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}
