// Float64 dB arithmetic shared by the kernels that turn magnitudes into dB (heal.hip, stft.hip's band-dB form,
// expander.hip): util/units.py:24-25 to_dB = 20 log10(a) evaluated on float64.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace par {

// log10 of a positive, finite, normal float64 (every magnitude here is >= 1e-7): exponent + 2 atanh((f - 1) / (f + 1)) on
// f in [1/sqrt 2, sqrt 2), nine odd terms; |error| <= 1e-15 against numpy's log10 over 1e-7 .. 1e6 (about a third of the
// instructions of the library routine, which is what k_inpaint_gain spent 60 % of its time in).  Anything else -- NaN, Inf,
// the reference's poison values -- goes to the library.
__device__ __forceinline__ double log10_pos(double t) {
  if (!(t >= 0x1p-1000 && t <= 0x1p1000)) return log10(t);
  const long long bits = __double_as_longlong(t);
  int e = (int)(bits >> 52) - 1023;
  double f = __longlong_as_double((bits & 0x000fffffffffffffll) | 0x3ff0000000000000ll);      // [1, 2)
  if (f > 1.4142135623730951) {
    f *= 0.5;
    e += 1;
  }
  const double num = f - 1.0, den = f + 1.0;                       // den in (1.7, 2.42)
  double r = __builtin_amdgcn_rcp(den);
  r = __builtin_fma(__builtin_fma(-den, r, 1.0), r, r);
  r = __builtin_fma(__builtin_fma(-den, r, 1.0), r, r);
  double sq = num * r;
  sq = __builtin_fma(__builtin_fma(-den, sq, num), r, sq);         // (f - 1) / (f + 1) to the last bit or so
  const double z = sq * sq;
  double p = 1.0 / 17.0;
  p = __builtin_fma(p, z, 1.0 / 15.0);
  p = __builtin_fma(p, z, 1.0 / 13.0);
  p = __builtin_fma(p, z, 1.0 / 11.0);
  p = __builtin_fma(p, z, 1.0 / 9.0);
  p = __builtin_fma(p, z, 1.0 / 7.0);
  p = __builtin_fma(p, z, 1.0 / 5.0);
  p = __builtin_fma(p, z, 1.0 / 3.0);
  const double two_s = sq + sq;
  const double lnf = __builtin_fma(two_s * z, p, two_s);
  return __builtin_fma((double)e, 0.30102999566398120, lnf * 0.43429448190325182);
}

}  // namespace par
