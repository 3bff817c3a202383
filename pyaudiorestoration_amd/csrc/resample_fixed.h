// Host-side pieces of the fixed-ratio resampler (resample_fixed.hip) that its stand-alone host check also calls.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>

namespace par {

constexpr int kRsP = 512;                  // table entries per zero crossing (resampy's precision = 9)
constexpr double kRsRolloff = 0.945;
constexpr int kRsMaxZeros = 64;

// The filter table for Z zero crossings, computed in float64: nat[j] = (win[j], delta[j]), j = 0..P*Z.  phase (may be null;
// filled for Z = 8 only, zeros otherwise): the same entries phase-major, row off = 0..P holds (win, delta) of taps
// off, off + P, ... in 20 floats (16 used).
void rs_build_table(int Z, std::vector<float2>* nat, std::vector<float>* phase);

}  // namespace par
