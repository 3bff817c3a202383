// numpy's complex64 absolute, shared by the renoiser gate (stft.hip) and K_hpss (hpss.hip): the float32 value np.abs gives, which
// numpy's SIMD loop computes as larger * sqrt(fma(r, r, 1)), r = smaller / larger, every step a correctly rounded float32
// operation (not hypotf: that differs from numpy by an ulp in about a quarter of all bins).  The division and sqrtf are the
// compiler's correctly rounded expansions (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt).  The _rn intrinsics of the
// HIP headers are NOT: without OCML_BASIC_ROUNDED_OPERATIONS they map to the native instructions, and the native square root
// is an ulp under numpy's in one bin of eight (NOTES.md, Renoiser: 8970 of 70 001 tied bins gated that numpy passes).
// Contraction off: the product must round before anything a caller adds to it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace par {

__device__ __forceinline__ float np_abs_c64(float re, float im) {
#pragma clang fp contract(off)
  const float ar = fabsf(re), ai = fabsf(im);
  if (ar == __builtin_inff() || ai == __builtin_inff()) return __builtin_inff();
  if (ar != ar || ai != ai) return __builtin_nanf("");
  const float larger = fmaxf(ar, ai), smaller = fminf(ar, ai);
  const float r = larger == 0.0f ? 0.0f : smaller / larger;
  return sqrtf(fmaf(r, r, 1.0f)) * larger;
}

}  // namespace par
