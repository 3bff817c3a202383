// Spectrogram image from a STORED magnitude spectrogram, and its colours (util/spectrum.py: Spectrum.update_data, set_clims,
// set_cmap).  k_peak_image is the composed route of the picture k_stft_peak_image (stft.hip) takes straight from the samples: it
// serves transform sizes above 16384 points, spectrograms that already exist, and is the fused kernel's yardstick.
// k_image_colorize turns the peak image into RGBA8 through a 256-entry table; it is separate from the transform so that new
// limits or colours cost nothing but this pass.
#include "par_common.h"
#include "db_math.h"
#include "image_tables.h"

namespace par {

// One thread per cell (column c, row r): the maximum over the column's frames inside this chunk and the row's bins, taken on the
// bit patterns (image_key) and maximised into the cell.  One thread owns a cell for the whole launch and launches on a stream
// follow each other, so the read-modify-write needs no atomic.  Neighbouring rows read neighbouring bins of a frame.
__global__ __launch_bounds__(256) void k_peak_image(const float* __restrict__ mag, int64_t mag_pitch, int bins, int64_t frame_first,
                                                    int64_t n_chunk, const int64_t* __restrict__ cols, const int32_t* __restrict__ rows,
                                                    int height, float* __restrict__ peak, int64_t pitch) {
  const int r = blockIdx.y * 256 + threadIdx.x;
  if (r >= height) return;
  const int64_t c = blockIdx.x;
  int64_t lo = cols[2 * c], hi = cols[2 * c + 1];
  lo = lo < frame_first ? frame_first : lo;
  hi = hi > frame_first + n_chunk ? frame_first + n_chunk : hi;
  int rl = rows[2 * r], rh = rows[2 * r + 1];
  rl = rl < 0 ? 0 : rl;
  rh = rh > bins ? bins : rh;
  if (lo >= hi || rl >= rh) return;
  uint32_t m = 0;
  for (int64_t f = lo; f < hi; ++f) {
    const float* p = mag + (f - frame_first) * mag_pitch;
    for (int b = rl; b < rh; ++b) {
      const uint32_t key = image_key(p[b]);
      m = key > m ? key : m;
    }
  }
  uint32_t* cell = reinterpret_cast<uint32_t*>(peak + c * pitch + r);
  if (m > *cell) *cell = m;
}

// A 16 x 16 tile of cells: read along the rows of a column (contiguous in the column-major peak image), written along the
// columns of a row (contiguous in the row-major RGBA image), exchanged through LDS as table indices (256 = no data).
__global__ __launch_bounds__(256) void k_image_colorize(const float* __restrict__ peak, int64_t width, int64_t height, int64_t pitch,
                                                        double vmin, double span, const uint32_t* __restrict__ lut,
                                                        uint32_t* __restrict__ out) {
  __shared__ int tile[16][17];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int64_t x0 = (int64_t)blockIdx.x * 16, y0 = (int64_t)blockIdx.y * 16;
  {
    const int64_t c = x0 + ty, r = y0 + tx;
    int idx = 256;
    if (c < width && r < height) {
      const float m = peak[c * pitch + r];
      if (m == m && m != 0.0f) {
        const double dB = 20.0 * log10_pos((double)m);
        double t = (dB - vmin) / span;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
        idx = (int)floor(t * 255.0 + 0.5);
      }
    }
    tile[ty][tx] = idx;
  }
  __syncthreads();
  const int64_t c = x0 + tx, r = y0 + ty;
  if (c < width && r < height) {
    const int idx = tile[tx][ty];
    out[r * width + c] = idx == 256 ? 0u : lut[idx];
  }
}

}  // namespace par

extern "C" {

int par_peak_image_f32(int device, const float* mag, int64_t mag_pitch, int64_t bins, int64_t n_frames, int64_t frame_first,
                       int64_t n_frames_chunk, const int64_t* cols, const int64_t* cols_host, const int32_t* rows,
                       const int32_t* rows_host, int64_t width, int64_t height, float* peak, int64_t pitch, void* stream) {
  using namespace par;
  PAR_REQUIRE(mag && cols && cols_host && rows && rows_host && peak, PAR_ERR_ARG, "par_peak_image_f32: null pointer");
  PAR_REQUIRE(bins >= 1 && bins < (1ll << 31) && mag_pitch >= bins && n_frames >= 0 && frame_first >= 0 && n_frames_chunk >= 0 &&
                  n_frames_chunk <= n_frames && frame_first <= n_frames - n_frames_chunk && width >= 1 && height >= 1 &&
                  width <= kImageMaxSide && height <= kImageMaxSide && pitch >= height,
              PAR_ERR_ARG, "par_peak_image_f32: bad sizes (bins %lld, pitch %lld, frames [%lld, %lld + %lld) of %lld, image %lld x %lld, pitch %lld)",
              (long long)bins, (long long)mag_pitch, (long long)frame_first, (long long)frame_first, (long long)n_frames_chunk,
              (long long)n_frames, (long long)width, (long long)height, (long long)pitch);
  ImagePlan plan;
  const int rc = image_check_tables("par_peak_image_f32", cols_host, rows_host, width, height, n_frames, bins, &plan);
  if (rc != PAR_OK) return rc;
  if (n_frames_chunk == 0) return PAR_OK;
  PAR_HIP_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_peak_image, dim3((unsigned)width, (unsigned)ceil_div(height, 256)), dim3(256), 0, as_stream(stream), mag, mag_pitch,
                     (int)bins, frame_first, n_frames_chunk, cols, rows, (int)height, peak, pitch);
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}

int par_image_colorize_u8(int device, const float* peak, int64_t width, int64_t height, int64_t pitch, double vmin, double vmax,
                          const uint8_t* lut, uint8_t* out, void* stream) {
  using namespace par;
  PAR_REQUIRE(peak && lut && out, PAR_ERR_ARG, "par_image_colorize_u8: null pointer");
  PAR_REQUIRE(width >= 1 && height >= 1 && width <= kImageMaxSide && height <= kImageMaxSide && pitch >= height, PAR_ERR_ARG,
              "par_image_colorize_u8: bad sizes (image %lld x %lld, pitch %lld)", (long long)width, (long long)height, (long long)pitch);
  PAR_REQUIRE(vmin < vmax && vmax - vmin <= 1.7e308, PAR_ERR_ARG, "par_image_colorize_u8: limits [%g, %g] are not an interval", vmin, vmax);
  PAR_REQUIRE(((uintptr_t)lut & 3) == 0 && ((uintptr_t)out & 3) == 0, PAR_ERR_ARG, "par_image_colorize_u8: lut or out is not 4-byte aligned");
  PAR_HIP_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_image_colorize, dim3((unsigned)ceil_div(width, 16), (unsigned)ceil_div(height, 16)), dim3(256), 0, as_stream(stream),
                     peak, width, height, pitch, vmin, vmax - vmin, reinterpret_cast<const uint32_t*>(lut),
                     reinterpret_cast<uint32_t*>(out));
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}

}  // extern "C"
