// The band and peak arithmetic of the Peak / Peak Track trackers, shared by K_track (track.hip: bands of a stored magnitude
// spectrogram) and k_stft_peak (stft.hip: bands of a frame that never leaves LDS).  Semantics (reference util/wow_detection.py):
// Track.freq_plus_tolerance :109-117, set_bin_limits :97-107, freq_2_bin :81-82, get_peak :119-134, is_peak :136-139;
// correlation.parabolic (util/correlation.py:42-46).  Band/bin arithmetic is float64 like the reference.
#pragma once
#include "par_common.h"
#include <math.h>

namespace par {

struct Band {
  int NL, NU;
  bool past_end;       // NU reached past the last bin before the clip (a numpy slice clips silently; a product with a
                       // full-length window does not)
};

__device__ __forceinline__ int freq_to_bin(double f, int fft_size, double sr, int bins) {
  long long b = llrint(f * (double)fft_size / sr);        // Python round(): half-to-even
  if (b > bins - 1) b = bins - 1;
  if (b < 1) b = 1;
  return (int)b;
}

__device__ __forceinline__ Band band_limits(double freq, double tol, int fft_size, double sr, int bins) {
  const double lf = log2(freq);
  double fL = exp2(lf - tol), fU = exp2(lf + tol);
  fL = fL > 1.0 ? fL : 1.0;                                // max(1.0, fL)
  fU = fU < sr / 2 ? fU : sr / 2;                          // min(sr/2, fU)
  Band b;
  b.NL = freq_to_bin(fL, fft_size, sr, bins);
  b.NU = freq_to_bin(fU, fft_size, sr, bins);
  while (b.NU - b.NL < 4) {                                // min_bins = 4
    b.NL -= 1;
    b.NU += 1;
  }
  // A band widened below bin 0 (both edges on bin 1: a frequency below the transform's resolution) is an EMPTY
  // numpy slice [-k:NU] in the reference, whose argmax raises; reported through `empty`, never silently clamped.
  b.past_end = b.NU > bins;
  if (b.NU > bins) b.NU = bins;
  return b;
}

// The tail of get_peak behind the argmax, on a frame whose bin k is at(k): the status bits, is_peak on the two neighbours (bin 0
// reads bin bins - 1 as its left one: Python's index -1), parabolic() in float64, bin -> Hz.  `at` reads memory in K_track and
// LDS in k_stft_peak; the expression is this one in both.
// status bits: 1 empty band (ValueError), 2 peak on the last bin: is_peak() reads fft_frame[peak_i + 1] (IndexError),
// 4 band widened past the last bin: window(NU - NL) * spectrum[NL:NU] does not broadcast (ValueError); freq_2_bin caps
// both edges at bins - 1 and min_bins is 4, so such a slice always keeps >= 3 bins against a window of >= 4
template <class At>
__device__ __forceinline__ double peak_refine(At at, int arg, Band b, int bins, int fft_size, double sr, int* __restrict__ status) {
  double x = (double)arg;
  if (b.past_end) {
    atomicOr(status, 4);
    return x / (double)fft_size * sr;
  }
  if (arg == bins - 1) {
    atomicOr(status, 2);
    return x / (double)fft_size * sr;
  }
  const double fm = (double)at((arg - 1 + bins) % bins), f0 = (double)at(arg), fp = (double)at(arg + 1);
  if (fm < f0 && f0 > fp) {
    // parabolic(): xv = 1/2*(f[x-1]-f[x+1]) / (f[x-1]-2f[x]+f[x+1]) + x
    x = 0.5 * (fm - fp) / (fm - 2.0 * f0 + fp) + x;
  }
  return x / (double)fft_size * sr;
}

__device__ __forceinline__ double peak_freq(const float* __restrict__ col, Band b, int bins, int fft_size, double sr,
                                            int* __restrict__ status) {
  int arg = b.NL;
  float best = col[b.NL];
  for (int k = b.NL + 1; k < b.NU; ++k) {
    const float v = col[k];
    if (v > best) {                                        // first occurrence of the maximum (np.argmax)
      best = v;
      arg = k;
    }
  }
  return peak_refine([&](int k) { return col[k]; }, arg, b, bins, fft_size, sr, status);
}

// Shared tail of the tracker entry points: read the status word back (one 4-byte copy; the callers need the traced freqs on the
// host anyway) and turn its bits into the reference's errors.
inline int check_empty(int* d_flag, hipStream_t s, const char* who) {
  int h = 0;
  PAR_HIP_CHECK(hipMemcpyAsync(&h, d_flag, sizeof(h), hipMemcpyDeviceToHost, s));
  PAR_HIP_CHECK(hipStreamSynchronize(s));
  PAR_REQUIRE(!(h & 1), PAR_ERR_EMPTY_BAND,
              "%s: a tracking band is empty (frequency below the transform's resolution: the reference's slice "
              "[NL:NU] with NL < 0 is empty and its argmax raises)", who);
  PAR_REQUIRE(!(h & 2), PAR_ERR_INDEX, "%s: the peak sits on the last bin (is_peak() reads fft_frame[peak_i + 1]: IndexError)", who);
  PAR_REQUIRE(!(h & 4), PAR_ERR_SHAPE, "%s: the band reaches past the last bin (operands could not be broadcast together: "
              "np.hanning(NU - NL) against the clipped slice)", who);
  return PAR_OK;
}

}  // namespace par
