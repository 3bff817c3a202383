// Which K_sinc a planned file gets: the one rule behind par_varispeed_fused_f32 / _stereo_f32 / _batch_f32 (include/par_hip.h,
// "Which kernel runs").  Host arithmetic on a par_fused_item, nothing of HIP: tests/sinc_route_table.cpp compiles this header
// alone and prints the rule as a table.
#pragma once
#include <stdint.h>
#include "../../include/par_hip.h"

namespace par {

enum class SincRoute {
  Block,          // the block kernel (k_sinc_fused): any NT, any strides, short files
  StreamMono,     // the streaming kernel (sinc2.hip) + tile list: a mono signal on unit strides
  StreamPick,     // ... ONE channel of a two-channel interleaved file (the reference's use_channels view), any output stride
  StreamStereo,   // ... both channels of an interleaved file
};

// The streaming kernel is built for NT = 32 and does a file's first tile and its last two the block kernel's way: below four
// 1024-output tiles nothing is left to stream, and its ring reads whole 128-sample chunks of input.
constexpr int64_t kSincStreamMin = 4096;        // outputs, and input samples

inline SincRoute sinc_route(const par_fused_item& f, int NT, bool stream_allowed) {
  if (NT != 32 || !stream_allowed || f.len_out < kSincStreamMin || f.len_in < kSincStreamMin) return SincRoute::Block;
  if (f.sig1 && f.out1) {
    const bool interleaved = f.sig_stride == 2 && f.out_stride == 2 && f.sig1 == f.sig0 + 1 && f.out1 == f.out0 + 1 &&
                             (reinterpret_cast<uintptr_t>(f.out0) & 7) == 0;     // (the stereo streams store 8-byte pairs)
    return interleaved ? SincRoute::StreamStereo : SincRoute::Block;
  }
  // one channel (a lone sig1 or out1 is not looked at)
  if (f.sig_stride == 1 && f.out_stride == 1) return SincRoute::StreamMono;
  if (f.sig_stride == 2 && f.out_stride >= 1) return SincRoute::StreamPick;
  return SincRoute::Block;
}

// Several files: StreamMono / StreamStereo when there are at least two and every one of them has that route -- their launches
// can be merged; Block otherwise: go item by item.
inline SincRoute sinc_batch_route(int n, const par_fused_item* items, int NT, bool stream_allowed) {
  if (n < 2) return SincRoute::Block;
  const SincRoute r = sinc_route(items[0], NT, stream_allowed);
  if (r != SincRoute::StreamMono && r != SincRoute::StreamStereo) return SincRoute::Block;
  for (int k = 1; k < n; ++k)
    if (sinc_route(items[k], NT, stream_allowed) != r) return SincRoute::Block;
  return r;
}

}  // namespace par
