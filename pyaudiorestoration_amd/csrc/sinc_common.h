// Pieces shared by the two K_sinc translation units (sinc.hip: block kernels; sinc2.hip: the streaming kernel).
#pragma once
#include "par_common.h"
#include "pos_plan.h"
#include "sinc_route.h"

namespace par {

// sin(pi*x), cos(pi*x) on [-0.5, 0.5]; Taylor in (pi*x), abs error < 1e-7 at the interval ends.
__device__ __forceinline__ float sinpi_half(float x) {
  const float z = x * x;
  float p = -0.00737043094f;               // -pi^11/11!
  p = fmaf(p, z, 0.0821458866f);           //  pi^9/9!
  p = fmaf(p, z, -0.599264529f);           // -pi^7/7!
  p = fmaf(p, z, 2.55016404f);             //  pi^5/5!
  p = fmaf(p, z, -5.16771278f);            // -pi^3/3!
  p = fmaf(p, z, 3.14159265f);             //  pi
  return p * x;
}
__device__ __forceinline__ float cospi_half(float x) {
  const float z = x * x;
  float p = 0.00192957431f;                //  pi^12/12!
  p = fmaf(p, z, -0.0258068914f);          // -pi^10/10!
  p = fmaf(p, z, 0.235330630f);            //  pi^8/8!
  p = fmaf(p, z, -1.33526277f);            // -pi^6/6!
  p = fmaf(p, z, 4.05871213f);             //  pi^4/4!
  p = fmaf(p, z, -4.93480220f);            // -pi^2/2!
  p = fmaf(p, z, 1.0f);
  return p;
}

__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }

// What the fused kernels read of a plan (views into the caller's work / aux buffers, pos_plan.h).
struct FusedArgs {
  const double* speeds;
  const int64_t* seg_start;
  const double* seg_off;
  const double* ck;
  const int64_t* tile_seg;
  const SegFast* seg_fast;
  const TileHdr* hdr;
  const BlockRec* rec;
  const BlockRec2* rec2;
  int64_t nseg;
  int* redo_count;           // streaming kernel -> block kernel: tiles to do the old way ([0] = how many)
  int* redo_list;
};

// One file as the streaming launches and the tile lists see it: sig / out point at the first sample of the channel (StreamStereo:
// the left channel's; len_in / len_out count frames).  ListBatch (sinc.hip), a kernel argument, holds these: the member order stays.
struct SincFile {
  int64_t len_out, len_in;
  const float* sig;
  float* out;
  FusedArgs fa;
};

// Streaming kernel (sinc2.hip), NT = 32, in the form the route names (sinc_route.h) -- StreamMono: a mono signal on unit strides;
// StreamStereo: an interleaved stereo file; StreamPick: ONE channel of a two-channel interleaved file (input stride 2; outputs
// pick_out_stride elements apart, read for this route only).  Tiles it does not take are appended to fa.redo_list.
struct TapModes;
int launch_sinc_stream(int device, SincRoute route, const SincFile& f, int64_t pick_out_stride, const float4* tab, const TapModes& tmd,
                       hipStream_t s);

// ... and several files of one route (StreamMono or StreamStereo) in one launch per kernel kind (k_sinc_pipe_n; at most kFusedBatchMax)
constexpr int kFusedBatchMax = 8;
int launch_sinc_stream_batch(int device, SincRoute route, int n, const SincFile* files, const float4* tab, const TapModes& tmd, hipStream_t s);

}  // namespace par
