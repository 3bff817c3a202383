// Pixel tables of the spectrogram image, shared by stft.hip (k_stft_peak_image, straight from the samples) and image.hip
// (k_peak_image on a stored spectrogram, k_image_colorize).  A column is a half-open frame range (int64 lo, hi), a row a half-open
// bin range (int32 lo, hi); both arrive as a DEVICE array the kernels read and a HOST copy the calls validate and size from.
#pragma once
#include "par_common.h"

namespace par {

constexpr int64_t kImageMaxSide = 1 << 19;       // pixels per side an image call takes (PAR_IMAGE_MAX_SIDE)
constexpr int64_t kImageMinRun = 16;             // frames per chunk of a column at the least: 16 transforms amortise a column of rows
constexpr int64_t kImageMaxUnits = 16384;        // aimed-at (column, chunk) units of a long file: eight rounds of the device's frame slots

// A float32 magnitude as the unsigned integer the maxima are taken on: positive floats order as their bit patterns do, and every
// NaN becomes the one pattern above them all (a NaN that arrives with its sign bit set would otherwise lose against everything).
__host__ __device__ inline uint32_t image_key(float m) {
  union {
    float f;
    uint32_t u;
  } v;
  v.f = m;
  return m != m ? 0x7fc00000u : v.u;
}

// frames per chunk: depends on the tables alone (the frames the distinct columns name), never on the device
inline int64_t image_chunk_len(int64_t named_frames) {
  const int64_t r = ceil_div(named_frames, kImageMaxUnits);
  return r < kImageMinRun ? kImageMinRun : r;
}

struct ImagePlan {
  int64_t named_frames = 0;    // frames of the distinct, non-empty columns
  int64_t chunk = 0;           // image_chunk_len(named_frames)
  int64_t n_units = 0;         // (distinct column, chunk) pairs
  int64_t passes = 0;          // frames of the longest chunk
};

// Validates both tables against [0, n_frames] x [0, bins] and plans the fused launch.  Host only, no device call.
inline int image_check_tables(const char* who, const int64_t* cols_host, const int32_t* rows_host, int64_t width, int64_t height,
                              int64_t n_frames, int64_t bins, ImagePlan* plan) {
  int64_t row_sum = 0;
  for (int64_t r = 0; r < height; ++r) {
    const int64_t lo = rows_host[2 * r], hi = rows_host[2 * r + 1];
    PAR_REQUIRE(lo >= 0 && lo <= hi && hi <= bins, PAR_ERR_ARG, "%s: row %lld is bins [%lld, %lld) of %lld", who, (long long)r,
                (long long)lo, (long long)hi, (long long)bins);
    row_sum += hi - lo;
  }
  PAR_REQUIRE(row_sum <= bins + height, PAR_ERR_ARG, "%s: the rows name %lld bins, more than bins + height = %lld", who,
              (long long)row_sum, (long long)(bins + height));
  ImagePlan p;
  for (int64_t c = 0; c < width; ++c) {
    const int64_t lo = cols_host[2 * c], hi = cols_host[2 * c + 1];
    PAR_REQUIRE(lo >= 0 && lo <= hi && hi <= n_frames, PAR_ERR_ARG, "%s: column %lld is frames [%lld, %lld) of %lld", who, (long long)c,
                (long long)lo, (long long)hi, (long long)n_frames);
    if (c > 0) {
      const int64_t plo = cols_host[2 * c - 2], phi = cols_host[2 * c - 1];
      const bool same = lo == plo && hi == phi;
      PAR_REQUIRE(same || lo >= phi, PAR_ERR_ARG, "%s: column %lld [%lld, %lld) overlaps its predecessor [%lld, %lld) without being equal to it",
                  who, (long long)c, (long long)lo, (long long)hi, (long long)plo, (long long)phi);
      if (same) continue;
    }
    p.named_frames += hi - lo;
  }
  p.chunk = image_chunk_len(p.named_frames);
  for (int64_t c = 0; c < width; ++c) {
    const int64_t lo = cols_host[2 * c], hi = cols_host[2 * c + 1];
    if (hi == lo || (c > 0 && lo == cols_host[2 * c - 2] && hi == cols_host[2 * c - 1])) continue;
    const int64_t nc = ceil_div(hi - lo, p.chunk), longest = ceil_div(hi - lo, nc);
    p.n_units += nc;
    if (longest > p.passes) p.passes = longest;
  }
  *plan = p;
  return PAR_OK;
}

}  // namespace par
