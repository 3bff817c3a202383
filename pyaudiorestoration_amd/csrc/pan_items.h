// Work items of the stereo balance measurement, shared by pan.hip (boxes on spectrograms) and stft.hip (k_stft_pan, boxes
// straight from the two channels): one item per (box, frame), one (sum, count) pair per item in the caller's scratch.
#pragma once
#include "par_common.h"

namespace par {

struct PanPart {
  double sum;        // float64 sum of the item's float32 quotients that are not NaN
  long long cnt;     // how many those were
};

constexpr int64_t kPanMaxBoxes = 65535;

// box = (bin_l, bin_u, frame_0, frame_1), half-open: an item per frame when the box holds a cell at all
__host__ __device__ inline int64_t pan_box_items(const int* bx) {
  return (bx[1] > bx[0] && bx[3] > bx[2]) ? (int64_t)bx[3] - bx[2] : 0;
}

// the box an item belongs to: the last b with offs[b] <= item (empty boxes share their successor's offset and are passed over)
__device__ __forceinline__ int64_t pan_item_box(const int64_t* __restrict__ offs, int64_t n_box, int64_t item) {
  int64_t lo = 0, hi = n_box;                     // offs[lo] <= item < offs[hi]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (offs[mid] <= item) lo = mid; else hi = mid;
  }
  return lo;
}

inline size_t pan_offs_bytes(int64_t n_box) { return ((size_t)(n_box + 1) * sizeof(int64_t) + 15) & ~(size_t)15; }

// pan.hip
size_t pan_scratch_bytes(const int32_t* boxes_host, int64_t n_box);
int pan_check_boxes(const char* who, const int32_t* boxes_host, int64_t n_box, int64_t bins, int64_t n_frames, int64_t* n_items);
void launch_pan_offsets(const int* boxes, int64_t n_box, void* scratch, hipStream_t s);
void launch_pan_reduce(int64_t n_box, const void* scratch, double* fac, int64_t* count, hipStream_t s);

}  // namespace par
