/*
 * par_hip.h -- C ABI of libpar_hip.so, the MI355X (gfx950) implementation of the
 * pyaudiorestoration util/ hot path.  This is the drop-in boundary: plain pointers
 * and sizes, no torch / numpy / C++ types.  Every DEVICE pointer is caller-owned
 * HBM (the Python host layer allocates it through torch-ROCm tensors); `stream`
 * is a hipStream_t passed as void* (NULL = the default stream).  The library keeps
 * no global state except small per-device constant tables (twiddles, sinc tap
 * tables, the fixed-ratio resampler's filter table) keyed by (device, size).
 *
 * All functions return an int status (0 = PAR_OK), never throw, and record a
 * message retrievable with par_last_error() (thread-local).  Functions are
 * re-entrant and call hipSetDevice(device) themselves, so they may be driven from
 * one host thread per GPU (ctypes releases the GIL).
 *
 * Citations are file:line in the reference checkout (HENDRIX-ZT2/pyaudiorestoration).
 */
#ifndef PAR_HIP_H
#define PAR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PAR_OK 0
#define PAR_ERR_ARG 1            /* bad argument (the reference would raise or misbehave) */
#define PAR_ERR_HIP 2            /* a HIP runtime call failed */
#define PAR_ERR_UNSUPPORTED 3    /* valid for the reference, not implemented here (caller falls through) */
#define PAR_ERR_WORKSPACE 4      /* caller-provided workspace too small */
#define PAR_ERR_EMPTY_BAND 5     /* a tracker band is empty: the reference raises ValueError (argmax of an empty slice) */
#define PAR_ERR_INDEX 6          /* the reference indexes past the end of an array here and raises IndexError */
#define PAR_ERR_SHAPE 7          /* the reference multiplies arrays of different lengths here and raises ValueError */

/* ---- library / device ---------------------------------------------------------- */
int par_version(void);
int par_device_count(void);
int par_last_error(char* buf, int n);
/* stream-ordered helper used by the host layer and bench to time kernels with HIP events
 * on the stream the kernels are launched on (torch.cuda.Event only sees torch's stream). */
int par_event_create(void** ev);
int par_event_destroy(void* ev);
int par_event_record(void* ev, void* stream);
int par_event_elapsed_ms(void* start, void* stop, float* ms);   /* synchronises on `stop` */
int par_stream_sync(int device, void* stream);
/* A side stream for the plan of the next file (resampling.varispeed_batch_dev, bench.py): cu_count > 0 confines its kernels
 * to the first cu_count compute units (hipExtStreamCreateWithCUMask), otherwise low_priority != 0 asks for the device's
 * least stream priority.  Wrap the handle with torch.cuda.ExternalStream; destroy it with par_stream_destroy. */
int par_stream_create(int device, int low_priority, int cu_count, void** stream);
int par_stream_destroy(void* stream);

/* ---- S0-S4: STFT / magnitude ---------------------------------------------------
 * Replaces the backend slot of util/fourier.py:67-75, i.e. a callable
 * (n_fft, step, window, x, zeropad) like pyfftw_rfft2 (:124-133) / np_rfft_pick (:136-157):
 * reflect-pad n_fft/2 (estimate_and_center :78-82), frame i = window * xpad[i*hop : i*hop+n_fft]
 * zero-extended at the END to n_fft*zeropad (segment_array :160-166), real FFT, / sqrt(n_fft)
 * (numpy/torch normalisation).  mode 1 fuses to_mag (:23-24): |X| + 1e-7.
 *
 *   x        device f32, logical length n, element stride x_stride (channel view of an (n,ch) array)
 *   window   device f32[n_fft] (scipy.signal.get_window(name, n_fft) as float32, :66)
 *   out      device, FRAME-MAJOR: mode 0 -> complex64 [frames][bins] interleaved re,im
 *                                 mode 1 -> float32   [frames][bins]
 *            bins = n_fft*zeropad/2+1, frames = par_stft_frames(n, n_fft, hop)
 * n_fft*zeropad must be a power of two in [16, 16384] (larger: par_stft_big_f32); otherwise PAR_ERR_UNSUPPORTED.
 */
int64_t par_stft_frames(int64_t n, int n_fft, int hop);
/* out_pitch (r03): elements (float, or float2 for mode 0) from one frame's row to the next; 0 = bins (packed rows).  A pitch
 * that is a multiple of 32 floats starts every magnitude row on a 128-byte line: a 513-bin row is 2052 bytes, packed rows
 * straddle lines at both ends and the streaming stores of neighbouring frames wrote 1.21x the bytes (WRITE_SIZE, r02). */
int par_stft_f32(int device, const float* x, int64_t n, int64_t x_stride, int n_fft, int hop, int zeropad,
                 const float* window, float* out, int mode, int64_t out_pitch, void* stream);

/* The same transform for frames of more than 8192 points (n_fft*zeropad a power of two in (8192, 2^24]; the GUI offers
 * FFT sizes up to 2^20 with zero-padding up to 16, util/widgets.py:333-351): up to 2^21 points a four-step FFT in two
 * passes over HBM (columns, then rows fused with the real-transform untangle: only one H-point array per frame is ever
 * stored); 2^22 .. 2^24 points (r03) as 2, 4 or 8 decimated 2^20-point sequences through that transform, recombined and
 * untangled bin by bin, a frame at a time (scratch: two H-point arrays).
 *   scratch  device memory of par_stft_big_scratch_bytes(n, n_fft, hop, zeropad) bytes (caller-owned) */
size_t par_stft_big_scratch_bytes(int64_t n, int n_fft, int hop, int zeropad);
int par_stft_big_f32(int device, const float* x, int64_t n, int64_t x_stride, int n_fft, int hop, int zeropad,
                     const float* window, float* out, int mode, void* scratch, size_t scratch_bytes, void* stream);

/* ---- S6: ISTFT -----------------------------------------------------------------
 * Replaces util/fourier.py:314-437 (istft, center=True, win_length=n_fft) incl.
 * window_sumsquare (:492-546) and __overlap_add (:677-687).  Does NOT mutate `spec`.
 *   spec     device complex64 [n_frames][bins] frame-major (bins = n_fft/2+1)
 *   window   device f32[n_fft]  (get_window(name, n_fft, fftbins=True))
 *   frames   device f32 scratch of par_istft_scratch_floats(n_frames, n_fft, hop) floats; that is 0 (pass NULL)
 *            when the frames are overlap-added in LDS and never stored (n_fft <= 2048 and the overlap-add span of
 *            one workgroup fits 64 KB), else [n_frames][n_fft] (n_fft >= 4096: a frame fills the workgroup alone and the
 *            fused form would re-transform n_fft/hop frames per hop of output); n_fft > 8192 (to 2^21: the GUI's FFT sizes go
 *            to 2^20, util/widgets.py:334-351): the frame array plus two complex arrays of the four-step transform
 *   y        device f32[y_len]; y[t] = ola[t + skip] / sumsq[t + skip] (0 beyond the ola length),
 *            skip = n_fft/2 and y_len = `length` reproduce fix_length(y[n_fft//2:], length) (:430-435).
 */
int64_t par_istft_scratch_floats(int64_t n_frames, int n_fft, int hop);
int par_istft_f32(int device, const float* spec, int64_t n_frames, int n_fft, int hop, const float* window,
                  float* frames, float* y, int64_t y_len, int64_t skip, void* stream);

/* Spectral gain mask of the dropout healer (dropout_healer_gui.py:161-162, util/units.py:28-29 to_fac):
 * spec[i] *= 10^(gain_db[i]/20) for a frame-major complex64 spectrogram and a float32 mask of `count` bins. */
int par_spec_apply_gain_db_c64(int device, float* spec, const float* gain_db, int64_t count, void* stream);

/* Sparse dropout healing (r03; dropout_healer_gui.py:111-166 touches only the marked boxes, and STFT -> ISTFT is the
 * identity elsewhere): copies `n_seg` sample ranges between two signals, dst[dst_start[k] + i] = src(src_start[k] + i)
 * for i < len[k].  run_start[k] = sum of len[0..k) (exclusive prefix), total = sum of len.  padded != 0: the source is the
 * reference's fix_length(signal, n_padded) (zeros from sample n_valid on, :120) under the STFT's np.pad(.., 'reflect')
 * (util/fourier.py:78-82), so a range may start before sample 0 or end behind n_padded.  All index arrays on the device. */
int par_copy_segments_f32(int device, const float* src, int64_t src_stride, int64_t n_valid, int64_t n_padded, int padded,
                          const int64_t* src_start, const int64_t* dst_start, const int64_t* len, const int64_t* run_start,
                          int64_t n_seg, int64_t total, float* dst, int64_t dst_stride, void* stream);
/* Gain mask of the dropout healer for a BATCH of markers (dropout_healer_gui.py:135-159): for each marker
 * (frame_b, frame_a, fs, bin_l, bin_u -- int32[n_markers][5] in device memory, the integers the reference
 * derives at :136-142) the mean dB of the fs frames before/after the box per bin, the linear fill across the
 * box (:149-153), gain = target - dB (:155) and np.clip(gain, previous, 255) (:157) folded into the mask.
 *   spec     device complex64 [n_frames][bins], frame-major (par_stft_f32 output); read only
 *   gain_db  device f32 [n_frames][bins], zero-initialised by the caller; updated with an atomic max, which
 *            equals the reference's marker-by-marker clip because the mask is non-negative (heal.hip header)
 * A marker whose box or surrounding frames leave the spectrogram contributes nothing.  A NaN gain (a NaN in a surrounding
 * frame, or Inf * 0 at the box's end) stays NaN like np.clip's, whatever other markers cover the bin. */
int par_inpaint_gain_db_c64(int device, const float* spec, int64_t n_frames, int64_t bins, const int32_t* markers,
                            int64_t n_markers, float* gain_db, void* stream);

/* Apply the mask over the marker boxes only and clear it (dropout_healer_gui.py:161-162 restricted to where the
 * mask can be non-zero): spec[i] *= 10^(gain_db[i]/20), gain_db[i] = 0 for every bin of every box; a bin inside
 * several boxes is scaled once.  `markers` as for par_inpaint_gain_db_c64.  Leaves gain_db all zeros, ready for
 * the next file, so a batch driver zero-fills the mask once per allocation, not once per file. */
int par_spec_apply_gain_boxes_c64(int device, float* spec, int64_t n_frames, int64_t bins, const int32_t* markers,
                                  int64_t n_markers, float* gain_db, void* stream);

/* Band volume curve of the dropout detector (dropout_healer_gui.py:195-203):
 * out[i] = mean_b 20*log10(mag[frame_b+i][b]), b in [bin_l, bin_u), i in [0, frame_a-frame_b); f64 out.
 *   mag  device f32 [n_frames][bins] frame-major magnitude (get_mag output, already + 1e-7). */
int par_band_mean_db_f32(int device, const float* mag, int64_t n_frames, int64_t bins, int64_t mag_pitch, int bin_l, int bin_u,
                         int64_t frame_b, int64_t frame_a, double* out, void* stream);

/* Heuristic dropout repair (dropouts_gui.MainWindow.process_heuristic, dropouts_gui.py:241-323): the two O(n) passes around
 * the band-pass of a band, over the n_ch channels of an interleaved (n, sig_stride) float32 file at once.
 *   par_curve_scale_f64:    out[c][i] = sig[i][c] * np.interp(np.linspace(0, 1, n)[i], np.linspace(0, 1, frames), fac[c])  (:314-317;
 *                           fac device f64[n_ch][frames] = correction factor - 1, out device f64[n_ch][n])
 *   par_accumulate_f64_f32: sig[i][c] = float32(float64(sig[i][c]) + y[c][i])                                                (:319-321) */
int par_curve_scale_f64(int device, const float* sig, int64_t sig_stride, int n_ch, int64_t n, const double* fac, int64_t frames,
                        double* out, void* stream);
int par_accumulate_f64_f32(int device, float* sig, int64_t sig_stride, int n_ch, int64_t n, const double* y, void* stream);

/* ---- R1: speed curve -> fractional read positions ----------------------------------
 * Replaces resampling.speed_to_pos (util/resampling.py:93-137).  Two calls because the
 * caller must allocate the position array:
 *   plan : segment lengths n_i (error-diffused rounding :111-118), per-segment reciprocal sums,
 *          the float64 offset chain (:125-126) and the end-trim (:129-135).  Returns len_out
 *          (= the written prefix when no trim fires) and whether the trim fired.
 *          Synchronises `stream`.
 *   fill : writes pos[0..len_out) as float64, bit-identical to the reference's array.
 * sampletimes/speeds are DEVICE float64[m].  work is caller-owned device scratch of at least
 * par_speed_plan_bytes(m) bytes and must stay untouched between plan and fill (or the fused
 * resampler below).
 * Curves with FEW points (segments of thousands of samples and more -- a constant speed correction is two points):
 * use par_speed_to_pos_plan_fused + par_speed_to_pos_fill_fused.  This plain form walks every segment on one lane
 * (seconds for a 10^8-sample segment); the fused plan's checkpoint buffer is what lets long segments be cut into
 * chunks whose float64 cumsum chain is evaluated exactly in parallel.
 */
size_t par_speed_plan_bytes(int64_t m);
int par_speed_to_pos_plan(int device, const double* sampletimes, const double* speeds, int64_t m, int64_t n_in,
                          void* work, size_t work_bytes, int64_t* len_out, int* trimmed, void* stream);
/* Same as par_speed_to_pos_plan; force_host != 0 runs the serial host evaluation of the two
 * order-dependent chains (the exact fallback the device scans defer to when they flag a near-tie),
 * *path_used (optional) reports 0 = device scans, 1 = serial host path, 2 = segment lengths redone on the host after a
 * near-tie (O(m)) with everything else on the device.  force_host == 2 (fused form, tests only) additionally injects
 * the failure the exact chunked cumsum reports when its verification does not close: the plan stays valid, *fused_ok
 * must come back 0. */
int par_speed_to_pos_plan_ex(int device, const double* sampletimes, const double* speeds, int64_t m, int64_t n_in,
                             void* work, size_t work_bytes, int64_t* len_out, int* trimmed, int force_host,
                             int* path_used, void* stream);
/* Why this thread's most recent plan left the device path: the device scans' flag word (1 near-tie in the segment
 * lengths, 2 some n_i < 2, 4 a_i outside the exact fixed-point range, 8 offset-chain verification failed, 16 more
 * binade crossings than the stitch table holds, 64 end_guess within the device sum's error of an integer); 0 when the
 * plan ran on the device (path_used 0; 64 alone is settled on the side and leaves the plan there) or the host path was
 * forced.  Diagnostics only. */
int par_last_plan_flags(void);
int par_speed_to_pos_fill(int device, const double* speeds, int64_t m, const void* work,
                          double* pos, int64_t len_out, void* stream);
/* The same fill from a FUSED plan (fused_ok): parallel over 8-sample blocks restarting from the cumsum checkpoints,
 * so a curve with a handful of points (segments of 10^7..10^9 samples) fills in milliseconds; bit-identical. */
int par_speed_to_pos_fill_fused(int device, const double* speeds, int64_t m, const void* work, const void* aux,
                                int64_t max_out, double* pos, int64_t len_out, void* stream);

/* ---- R2/R3: windowed-sinc varispeed interpolation --------------------------------------
 * Replaces sinc_wrapper / sinc_wrapper_mt / sinc_core (util/resampling.py:21-90), operator
 * slot #2: out[i] = sum_k signal[lower+k] * sinc((N_k-shift)*fc)*fc * hanning(2NT+1)[k].
 * Canonical period definition: period_to[i] = max(1e-12, pos[i+1]-pos[i])
 * for all but the global last sample (which reuses the previous one) == single-thread
 * sinc_wrapper.  Bug-compatible leading edge (quirk 1).  len_out >= 2, 1 <= NT <= 512.
 *   pos   device f64[len_out];  sig device f32 (len_in, stride sig_stride);
 *   out   device f32 (len_out, stride out_stride)  -- strided column views of (n,ch) arrays.
 * Positions may be ANY finite float64 (non-monotonic, repeated, negative, past the end, beyond the int64 range):
 * the window is clipped like the reference's slice signal[max(0, ind-NT) : min(ind+NT, len)], an empty slice
 * sums to 0.  Non-finite positions make the reference raise (int(round(p))); the Python mirror checks for them,
 * this entry point leaves the corresponding outputs unspecified (0 or NaN).
 */
int par_sinc_resample_f32(int device, const double* pos, int64_t len_out, const float* sig, int64_t sig_stride,
                          int64_t len_in, int NT, float* out, int64_t out_stride, void* stream);

/* Higher-level slot of resampling.run (util/resampling.py:184, :225-227): positions + sinc interpolation of
 * one channel from a finished plan.  n_chunks > 1 pipelines the work in pieces (position fill of chunk c+1
 * on a library-owned side stream while chunk c is interpolated); 0 = auto (= 1 on MI355X, where the overlap
 * measured no gain).  Bit-identical to par_speed_to_pos_fill + par_sinc_resample_f32.  pos is caller-owned f64[len_out]
 * scratch (it holds the reference's sample_at array afterwards). */
int par_varispeed_resample_f32(int device, const double* speeds, int64_t m, const void* work, int64_t len_out,
                               double* pos, const float* sig, int64_t sig_stride, int64_t len_in, int NT, float* out,
                               int64_t out_stride, int n_chunks, void* stream);
/* Fused resampler: positions never touch HBM.  par_speed_to_pos_plan_fused is par_speed_to_pos_plan_ex plus, in the
 * caller-owned device buffer `aux` (>= par_fused_aux_bytes(max_out, m) bytes, max_out >= len_out, e.g. 1.02*n_in), a
 * checkpoint of every segment's running reciprocal sum every 8 steps and a tile -> segment map.
 * par_varispeed_fused_f32 then runs K_sinc with each workgroup regenerating its tile's float64 positions in LDS
 * from those checkpoints (sequential float64 adds, bit-identical to numpy's cumsum) -- same output as
 * par_speed_to_pos_fill + par_sinc_resample_f32, 16 B/sample less HBM traffic.  *fused_ok (optional) reports
 * whether the checkpoints of every needed segment fit in aux; only then may par_varispeed_fused_f32 be called
 * (with the same work/aux/max_out and the returned len_out -- it does not read the plan back, so that it never
 * synchronises); otherwise callers use the position-array path (the plan itself stays valid).
 * LAZY plans (r05, csrc/pos_plan.h): on a dense, gentle curve (every segment 2..1024 outputs, speeds in [1/16, 64] changing
 * by <= 2^-9 of themselves across it) the plan skips the per-sample cumsum: segment sums in closed form with a rigorous error
 * bound, the exact sequential sum only for the few thousand segments where that bound could change a rounding of the offset
 * chain, and K_sinc walks a segment's cumsum with the reference's own arithmetic only for the ~1 output in 10^6 whose
 * position lies within the bound of a half-integer.  Offsets, len_out, trim and every window centre are bit-identical to
 * the eager plan's; *fused_ok comes back 2 and aux then holds NO checkpoints (par_speed_to_pos_fill_fused must not be used).
 * Curves that do not qualify are planned the eager way (*fused_ok 1).  force_host | 8 asks for the eager plan outright. */
size_t par_fused_aux_bytes(int64_t max_out, int64_t m);
int par_speed_to_pos_plan_fused(int device, const double* sampletimes, const double* speeds, int64_t m, int64_t n_in,
                                void* work, size_t work_bytes, void* aux, size_t aux_bytes, int64_t max_out,
                                int64_t* len_out, int* trimmed, int force_host, int* path_used, int* fused_ok,
                                void* stream);
int par_varispeed_fused_f32(int device, const double* speeds, int64_t m, const void* work, const void* aux,
                            int64_t max_out, int64_t len_out, const float* sig, int64_t sig_stride, int64_t len_in,
                            int NT, float* out, int64_t out_stride, void* stream);

/* Which kernel runs: NT = 32 files of at least four 1024-output tiles and 4096 input samples -- mono on unit strides, ONE
 * channel of a two-channel interleaved file (sig_stride == 2, any out_stride: the reference's use_channels column views,
 * util/resampling.py:211-227; r06), or (par_varispeed_fused_stereo_f32) the two channels of an INTERLEAVED file (sig1 = sig0 + 1,
 * out1 = out0 + 1, strides 2, out0 8-byte aligned) -- take the streaming kernel (csrc/sinc2.hip: one wave per 9-23 tiles, the taps |n| >= 3 of both tap regimes
 * as fixed filter banks on the matrix cores, fc < 1 through seven moment filters; stereo: one placement for both channels).  The
 * file's end tiles (first, last two, the partial one) are done the block kernel's way by the first workgroups of the same
 * launch; tiles the streams do not cover -- blocks outside the record model, window-centre ties, input float16 does not suit --
 * go to the block kernel (csrc/sinc.hip, sinc_block.h) through a tile list in `aux`.  Everything else (other NT, channels of
 * files with three or more channels, planar channel pairs, short files) takes the block kernel.  Results agree within the contract's tolerance and every window
 * centre is the reference's either way.  K_sinc WRITES that list into `aux`: one par_varispeed_fused_* launch per plan at a time
 * (two launches of one plan on different streams would race on it). */

/* Process-wide choice of that kernel, for tests and A/B sessions: form -1 = the default above, 0 = the block kernel for
 * everything.  Returns the previous setting. */
int par_debug_sinc_kernel(int form);

/* Diagnostic: how many 1024-output tiles of the LAST par_varispeed_fused_* launch on this aux buffer the streaming kernel
 * handed to the block kernel's tile list (blocks outside the record model, window-centre ties, input that float16 does not
 * suit).  Synchronises the stream.  0 when the streaming kernel did not run (the plan zeroes the count). */
int par_fused_redo_tiles(int device, const void* aux, int64_t max_out, int64_t m, int* tiles, void* stream);
/* ... and which tiles: *count = the length of that list, tiles[0 .. min(*count, cap)) = its entries (host buffer; the order is
 * the order in which the streams pushed them).  Tests aim their oracle windows at them.  Synchronises the stream. (ABI 105) */
int par_fused_redo_list(int device, const void* aux, int64_t max_out, int64_t m, int* tiles, int cap, int* count, void* stream);

/* Several planned files in ONE call (ABI 106; the reference loops over files, util/resampling.py:168, and an archive of short files
 * pays per file for the tails and gaps of the two or three kernels a file's K_sinc is): items that ALL take the streaming kernel in
 * one form -- NT = 32 and every item mono on unit strides, or every item an interleaved stereo file (sig1 = sig0 + 1, out1 = out0 + 1,
 * strides 2, out0 8-byte aligned) -- are launched merged, up to eight files per launch; any other mix is done item by item.
 * Outputs are bit-identical to par_varispeed_fused_f32 / par_varispeed_fused_stereo_f32 called per item (each file's streams are cut
 * as in its own launch).  sig1 == out1 == NULL: one channel.  Every item needs its own plan buffers (work, aux). */
typedef struct par_fused_item {
  const double* speeds;
  int64_t m;
  const void* work;
  const void* aux;
  int64_t max_out, len_out;
  const float* sig0;
  const float* sig1;
  int64_t sig_stride, len_in;
  float* out0;
  float* out1;
  int64_t out_stride;
} par_fused_item;
int par_varispeed_fused_batch_f32(int device, int n_items, const par_fused_item* items, int NT, void* stream);

/* Stereo form: two channels of ONE file (same positions; sig0/sig1 and out0/out1 share the strides -- e.g. the two
 * columns of an interleaved (n, 2) array: sig1 = sig0 + 1, stride 2) in one launch.  Outputs equal two
 * par_varispeed_fused_f32 calls to float32 rounding (the lane/output map differs); position regeneration, prologue and tap
 * weights are evaluated once for both.  Interleaved NT = 32 files take the streaming kernel's stereo form (see above). */
int par_varispeed_fused_stereo_f32(int device, const double* speeds, int64_t m, const void* work, const void* aux,
                                   int64_t max_out, int64_t len_out, const float* sig0, const float* sig1,
                                   int64_t sig_stride, int64_t len_in, int NT, float* out0, float* out1,
                                   int64_t out_stride, void* stream);

/* Profiling hook (bench.py roofline leg): HIP-event timing, on the caller's stream, of the K_sinc launches
 * issued by the last par_varispeed_resample_f32 call on `device`. */
int par_profile_enable(int device, int on);
int par_profile_read(int device, float* total_ms, int* launches, int64_t* samples);

/* "Linear" mode of resampling.run (util/resampling.py:229): np.interp(pos, arange(len), sig, 0, 0). */
int par_linear_resample_f32(int device, const double* pos, int64_t len_out, const float* sig, int64_t sig_stride,
                            int64_t len_in, float* out, int64_t out_stride, void* stream);

/* Lag-curve branch of resampling.run (util/resampling.py:189-206): pos = clip(np.interp(arange(num_out), xp, fp), 0),
 * cut at the first value >= len_signal (find_cutoff :265-270).  np.interp's operation order is kept (no FMA),
 * so positions are bit-identical.
 *   xp, fp   device f64[m], m >= 2: sampletimes and sampletimes - lags (samples)
 *   pos      device f64[num_out] (caller-allocated; only the first *len_out entries are meaningful)
 *   work     device scratch, >= 8 bytes
 *   len_out  host: num_out, or the cut-off index; *trimmed = 1 when the cut-off fired.  Synchronises the stream. */
int par_lag_to_pos_f64(int device, const double* xp, const double* fp, int64_t m, int64_t num_out, int64_t len_signal,
                       double* pos, void* work, int64_t* len_out, int* trimmed, void* stream);

/* ---- host-side codec: FLAC decoder standing in for soundfile/libsndfile (util/io_ops.py:7-16) ----
 * Pure host code, no GPU needed.  `data` is the whole file in host memory.
 *   par_flac_info        STREAMINFO fields; md5 (16 bytes, optional) is the stream's PCM signature
 *   par_flac_decode_f32  out: host float32 [total_frames][channels], scaled by 2^-(bits-1) like libsndfile's float
 *                        read; frame-parallel over n_threads (<= 0: all cores); every frame is CRC-checked;
 *                        verify_md5 != 0 also checks the decoded PCM against STREAMINFO's MD5. */
int par_flac_info(const void* data, size_t nbytes, int* sample_rate, int* channels, int* bits, int64_t* total_frames,
                  uint8_t* md5);
int par_flac_decode_f32(const void* data, size_t nbytes, float* out, int64_t frames_cap, int n_threads, int verify_md5,
                        int64_t* frames_decoded);

/* ---- synthetic workload generators, so bench inputs are born in HBM ---------- */
int par_synth_signal_f32(int device, float* out, int64_t start, int64_t count, double sr, uint64_t seed, void* stream);
int par_synth_speed_curve_f64(int device, double* sampletimes, double* speeds, int64_t m, double duration_s,
                              double sr, double depth, double rate_hz, double phase, void* stream);

/* ---- W1/W2: per-frame peak trackers on a device magnitude spectrogram ---------------------
 * Replaces the trace() loops of PeakTracker / PeakTrackTracker (util/wow_detection.py:294-327)
 * with Track.set_bin_limits (:97-107), get_peak (:119-134), is_peak (:136-139) and
 * correlation.parabolic (util/correlation.py:42-46).
 *   mag      device f32 frame-major [n_frames][bins], rows mag_pitch floats apart (0 = bins: packed; par_stft_f32's
 *            out_pitch).  The same parameter on par_track_cog_f64 / par_track_corr_f64 / par_piptrack_f32 /
 *            par_band_mean_db_f32.
 *   freqs    device f64[count]: in = sampled trail (sample_trail :66-76), out = traced frequencies
 *   mode 0   PeakTracker: band re-centred on freqs[i] every frame
 *   mode 1   PeakTrackTracker: band fixed on freqs[0]; tolerance halves for i > 2
 *   status   device int32 scratch (4 bytes).  A band whose widening reaches below bin 0 is an empty slice in the
 *            reference (its argmax raises ValueError): reported as PAR_ERR_EMPTY_BAND, never clamped; a peak on the last
 *            bin is its IndexError (is_peak reads the bin above): PAR_ERR_INDEX; a Center-of-Gravity band past the last
 *            bin is its broadcast ValueError: PAR_ERR_SHAPE.  Synchronises.
 */
int par_track_peak_f64(int device, const float* mag, int64_t n_frames, int bins, int64_t mag_pitch, int64_t frame_0,
                       int64_t count, double* freqs, int fft_size, double sr, double tolerance_oct, int mode, int32_t* status,
                       void* stream);
/* The same two trackers with the band magnitudes RE-EVALUATED FROM THE SIGNAL in float64 (r03): the reference's numpy
 * backend (util/fourier.py:136-157) hands Track.get_peak (util/wow_detection.py:119-134) float64 containers, and the
 * config-3 chain amplifies the float32 noise of a spectrogram into 3.7e-5 of the output peak.  Per frame only the band
 * [NL, NU) and the two neighbours of its peak are needed: a windowed direct DFT of the reference's own float32 frame
 * (reflect pad n_fft/2, sample x window rounded to float32: segment_array :160-166; zero-extended to n_fft * zeropad;
 * / sqrt(n_fft); + 1e-7 as to_mag :23-29 adds).
 *   x        device f32 signal channel, element stride x_stride, n samples;  window  device f32[n_fft]
 *   bins = n_fft * zeropad / 2 + 1, n_frames <= n / hop + 1; freqs / mode / status as par_track_peak_f64.
 * A band wider than 2048 bins: PAR_ERR_UNSUPPORTED (use par_track_peak_f64 on the spectrogram).  Synchronises. */
int par_track_peak_refined_f64(int device, const float* x, int64_t n, int64_t x_stride, int n_fft, int hop, int zeropad,
                               const float* window, int bins, int64_t n_frames, int64_t frame_0, int64_t count, double* freqs,
                               double sr, double tolerance_oct, int mode, int32_t* status, void* stream);
/* CenterOfGravity.trace (util/wow_detection.py:256-291): sequential band adaptation. */
int par_track_cog_f64(int device, const float* mag, int64_t n_frames, int bins, int64_t mag_pitch, int64_t frame_0, int64_t count,
                      double* freqs, int fft_size, double sr, double tolerance_oct, int32_t* status, void* stream);

/* W4: CorrelationTracker.trace (util/wow_detection.py:396-436) for all frames in one call: the band [NL, NU) of frames
 * 0 .. count-1 (the reference ignores frame_0 here) is resampled onto n = 4 (NU - NL) log2-frequency points by the
 * quadratic spline of scipy.interpolate.interp1d(kind='quadratic'), Hann-windowed, cross-correlated frame against next
 * frame (util/correlation.py:6-13, mode 'same'; the frame behind the last is all ones), peak refined by parabolic()
 * (:42-46), changes summed in order.
 *   M        device f64 [n][NU-NL] row-major: the spline as a matrix (band values -> grid values; the spline is linear
 *            in the data, the host applies scipy's own construction to the identity)
 *   wind     device f64 [n] = np.hanning(n)
 *   log_span = log2 f[NU-1] - log2 f[NL], log_mean = log2((fL + fU)/2): the reference's final scaling
 *   work     device f64 [par_track_corr_work_len(count, n)] = (count + 1) n + count.  On return it holds R[count + 1][n], the
 *            windowed resampled rows (row `count` = wind: the reference's all-ones frame), then changes[count] = n/2 - refined
 *            peak lag of rows i, i + 1 (NaN where a row's norm is 0: np.argmax returns the first NaN);  freqs  device f64 [count]
 *            out = exp2(log_mean + cumsum(changes) / n * log_span)
 *   status   device int32 scratch.  A peak on the last lag is the reference's IndexError: PAR_ERR_INDEX.  Synchronises.
 *   mag_pitch in (0, bins): PAR_ERR_ARG, here and in par_piptrack_f32, before any device call. */
/* PartialsTracker's librosa.piptrack (util/wow_detection.py:361-387; third-party routine, restated from librosa 0.10's
 * published source, parity unpinned): thresholded local maxima of every magnitude column inside [fmin, fmax), refined by
 * a parabola.  mag: device f32 [n_frames][bins] as par_stft_f32 mode 1 writes it; S = |(mag - offset) * scale| gives the
 * |stft| librosa works on (offset 1e-7, scale sqrt(n_fft)); piptrack takes |S| as librosa does (np.abs(S)), so a cell below
 * `offset` counts by its size.  bins may be less than fft_size / 2 + 1 (the lowest rows of the spectrum).  pitches / mags: device
 * f32 [n_frames][bins] out; mags round as numpy's float32 does (S + fl(fl(0.5 avg) shift): two roundings, no fused
 * multiply-add), and both maps equal the float32 restatement bit for bit.  NaN / inf magnitudes: unspecified. */
int par_piptrack_f32(int device, const float* mag, int64_t n_frames, int bins, int64_t mag_pitch, float scale, float offset, int fft_size,
                     double sr, double fmin, double fmax, float threshold, float* pitches, float* mags, void* stream);
int64_t par_track_corr_work_len(int64_t count, int n);
int par_track_corr_f64(int device, const float* mag, int64_t n_frames, int bins, int64_t mag_pitch, int NL, int NU, int64_t count,
                       const double* M, const double* wind, int n, double log_span, double log_mean, double* work,
                       double* freqs, int32_t* status, void* stream);

/* X2: util/correlation.py:6-39 on the device.  a, b: float64 device signals (what butter_bandpass_filter hands to
 * find_delay, pytapesynch_gui.py:128-131).
 *   par_xcorr_f64       scipy.signal.correlate(a/|a|, b/|b|, 'full'): full[na + nb - 1] float64, through one complex
 *                       float32 transform of a/|a| + i b/|b| (values carry ~1e-6; measured per transform size, and with
 *                       takes 80 dB apart in level, in tests/test_xcorr_gpu.py)
 *   par_find_delay_f64  find_delay(a, b, ignore_phase) with the window already applied by the caller (the reference
 *                       multiplies a and b in place): the peak of the 'same' correlation is located by the transform,
 *                       the lags around it are re-evaluated as float64 dot products and parabolic() (:42-46) runs on
 *                       those; *delay = peak - na//2 (host), *corr = its height.  A peak on the last lag is the
 *                       reference's IndexError: PAR_ERR_INDEX.  The call is par_find_delay_batch_f64's work on one row,
 *                       by the same kernels, decided on the device (the peak is sought in the float64 correlation
 *                       array, the same doubles a batch row reads out of its transform); it synchronises once, to
 *                       copy delay, corr and the row's status to the host.
 *                       Rival peaks: every local maximum of the transform's output within kXcRivalTol = 4.0e-6 of its
 *                       top, more than two lags from it, is re-evaluated exactly and the exact values decide (lowest
 *                       lag on a tie).  The exact argmax is certain to be listed while twice the transform's worst
 *                       error stays below kXcRivalTol.  Up to 63 rivals are decided; 64 or more are taken for a
 *                       plateau and the transform's own top stands.
 *   scratch             device bytes of par_xcorr_scratch_bytes(na, nb).  na + nb - 1 <= 2^20: one transform; longer signals
 *                       (up to 2^25 samples each, else PAR_ERR_UNSUPPORTED) are correlated in pairs of 2^19-sample sections */
size_t par_xcorr_scratch_bytes(int64_t na, int64_t nb);
int par_xcorr_f64(int device, const double* a, int64_t na, const double* b, int64_t nb, void* scratch, size_t scratch_bytes,
                  double* full, void* stream);
int par_find_delay_f64(int device, const double* a, int64_t na, const double* b, int64_t nb, int ignore_phase, void* scratch,
                       size_t scratch_bytes, double* delay, double* corr, void* stream);

/* X2 batch: the tape-sync tool's azimuth mode (pytapesynch_gui.py:210-238) cuts, filters and correlates one window pair per
 * dur/overlap seconds of a selection.  par_find_delay_batch_f64 and par_gather_windows_f64 are added at ABI 109:
 * par_version() stays 109.
 *   par_find_delay_batch_f64  find_delay for n_win pairs of rows of one shape: a DEVICE f64 [n_win][a_pitch] (na used),
 *                       b DEVICE f64 [n_win][b_pitch] (nb used).  win_a [na] / win_b [nb]: DEVICE f64 or NULL; when given,
 *                       every row is multiplied by its window IN PLACE first (util/correlation.py:18-20), so after the
 *                       call the rows hold row * win.  delay, corr: DEVICE f64 [n_win]; status: DEVICE int32 [n_win],
 *                       0 = ok, 1 = the peak sits on lag na - 1 (the reference's IndexError in parabolic()): delay and
 *                       corr of THAT row are NaN, every other row is computed.  A row of zeros has norm 0: delay and corr
 *                       are NaN with status 0, as the reference's division carries it.
 *                       The work per window -- norms, one packed float32 transform pair, first argmax, rivals within
 *                       kXcRivalTol re-decided exactly (64 or more: the transform's top stands), exact values at
 *                       peak-3 .. peak+3, numpy's f[-1] wrap at peak 0, parabolic() -- is decided on the device:
 *                       nothing is copied to the host and the call does not synchronise (a device's first call of a
 *                       transform size uploads its twiddles).  par_find_delay_f64 is this call's n_win = 1 through the
 *                       same kernels: a row's results do not depend on its neighbours, its pitch, n_win or the entry.
 *                       na + nb - 1 <= 2^20 (one transform per window), else PAR_ERR_UNSUPPORTED: loop over
 *                       par_find_delay_f64.  na < 3, nb < 1, n_win < 0, a pitch below its length, a null pointer:
 *                       PAR_ERR_ARG before any device call.  n_win == 0: PAR_OK, nothing done.
 *   scratch             DEVICE bytes.  par_find_delay_batch_scratch_bytes gives the size for all n_win windows in one pass,
 *                       capped at 32768 windows and at 1 GiB of transform arrays plus the per-window tables, never less than
 *                       one window's worth (0: the shape is unsupported).  Any size from one window's worth up is accepted
 *                       (less: PAR_ERR_WORKSPACE); the windows go through in passes of as many as it holds and the results
 *                       do not depend on it.
 *   par_gather_windows_f64  Spectrum.get_signal (util/spectrum.py:158-171) for n_win windows of one channel:
 *                       out[w * out_pitch + i] = (double)sig[(starts[w] + i - pad_l[w]) * sig_stride] for
 *                       pad_l[w] <= i < pad_l[w] + lens[w], 0.0 for every other i < n_out; nothing at i >= n_out.
 *                       sig: DEVICE f32, sample k of the channel at sig[k * sig_stride], n samples.  starts, lens, pad_l:
 *                       DEVICE int64 [n_win].  host_geom: HOST int64 [3][n_win] = the same starts, lens and pad_l rows, one
 *                       after the other; the call checks THESE before anything is launched: a window with a negative
 *                       field, starts + lens > n or pad_l + lens > n_out is PAR_ERR_ARG.  The kernel itself reads nothing
 *                       outside sig[0, n) whatever the device arrays hold. */
size_t par_find_delay_batch_scratch_bytes(int64_t na, int64_t nb, int64_t n_win);
int par_find_delay_batch_f64(int device, double* a, int64_t a_pitch, int64_t na, double* b, int64_t b_pitch, int64_t nb,
                             int64_t n_win, const double* win_a, const double* win_b, int ignore_phase, void* scratch,
                             size_t scratch_bytes, double* delay, double* corr, int32_t* status, void* stream);
int par_gather_windows_f64(int device, const float* sig, int64_t sig_stride, int64_t n, const int64_t* starts, const int64_t* lens,
                           const int64_t* pad_l, const int64_t* host_geom, int64_t n_win, int64_t n_out, double* out,
                           int64_t out_pitch, void* stream);

/* X2 sectioned batch: experiments/group_delay.py:30-96 correlates two WHOLE signals once per frequency band.
 * par_find_delay_sect_scratch_bytes and par_find_delay_sect_f64 are added at ABI 109: par_version() stays 109.
 *   par_find_delay_sect_f64  find_delay for n_win pairs of rows of one shape and any length: a DEVICE f64 [n_win][a_pitch]
 *                       (3 <= na <= 2^25 used), b DEVICE f64 [n_win][b_pitch] (1 <= nb <= 2^25 used).  The rows are only
 *                       read; windows are the caller's business.  delay, corr: DEVICE f64 [n_win]; status: DEVICE int32
 *                       [n_win], with par_find_delay_batch_f64's meaning (1 = peak on lag na - 1, that row NaN; a row of zeros
 *                       is NaN with status 0).  norms: DEVICE f64 [n_win][2] = (|a_w|, |b_w|) as the search used them, or
 *                       NULL.  same_out: DEVICE f64 [n_win][same_pitch] or NULL; when given, row w receives the na values
 *                       of the 'same' correlation as the transforms give them -- the very doubles the peak stage compares.
 *                       Rows are cut into sections of S = 2^section_log2 samples (12..19; 0 means 19), P = ceil(na / S) of a
 *                       and Q = ceil(nb / S) of b, transformed at N = 2 S points.  Section pairs with the same offset
 *                       d = p - q share one spectrum C_d = sum A_p conj(B_q): max(P, Q) transforms of the packed sections
 *                       and P + Q - 1 of the diagonals per row, instead of 2 P Q, and every row of a pass goes through the
 *                       same launches.  A lag receives at most two diagonals' values, added in float64 in a fixed order.
 *                       The search is par_find_delay_batch_f64's, by the same kernels: a row's (delay, corr, status) equals
 *                       par_find_delay_f64's bit for bit -- both end in the same exact sums over the same norms -- and does
 *                       not depend on section_log2, the pitches, n_win, the neighbouring rows or the scratch size, while
 *                       twice the route's worst lag error stays below kXcRivalTol (measured on same_out in
 *                       tests/test_xcorr_sect_gpu.py) and fewer than 64 rivals are listed.  Nothing is copied to the host and
 *                       the call does not synchronise (a device's first call of a transform size uploads its twiddles).
 *                       A null pointer (norms and same_out excepted), na < 3, nb < 1, n_win < 0, a pitch below its length,
 *                       section_log2 outside {0, 12..19}: PAR_ERR_ARG before any device call.  n_win == 0: PAR_OK, nothing
 *                       done.  A row above 2^25 samples: PAR_ERR_UNSUPPORTED.
 *   scratch             DEVICE bytes.  par_find_delay_sect_scratch_bytes gives the size for all n_win rows in one pass, capped
 *                       at 32768 rows and at 1 GiB of transform arrays plus the per-row tables, never less than one row's
 *                       worth (0: the shape is unsupported).  Any size from one row's worth up is accepted (less:
 *                       PAR_ERR_WORKSPACE); the rows go through in passes of as many as it holds. */
size_t par_find_delay_sect_scratch_bytes(int64_t na, int64_t nb, int64_t n_win, int section_log2);
int par_find_delay_sect_f64(int device, const double* a, int64_t a_pitch, int64_t na, const double* b, int64_t b_pitch, int64_t nb,
                            int64_t n_win, int section_log2, int ignore_phase, void* scratch, size_t scratch_bytes, double* delay,
                            double* corr, int32_t* status, double* norms, double* same_out, int64_t same_pitch, void* stream);

/* W3: sign-change indices of a (band-passed) float64 signal, ascending -- zero_crossings(a) =
 * np.where(np.bitwise_xor(a[1:] > 0, a[:-1] > 0))[0] (util/wow_detection.py:448-450), the full-rate pass of
 * ZeroCrossingTracker.trace (:340).
 *   work   device int64[par_zero_crossings_work_len(n)]
 *   idx    device int64[cap], or NULL to only count; *count (host) = number of crossings.  Synchronises the stream. */
int64_t par_zero_crossings_work_len(int64_t n);
int par_zero_crossings_f64(int device, const double* x, int64_t n, int64_t* work, int64_t* idx, int64_t cap, int64_t* count,
                           void* stream);

/* ---- F1: zero-phase SOS filtering ------------------------------------------------------
 * Replaces scipy.signal.sosfiltfilt(sos, data) as called by butter_bandpass_filter
 * (util/filters.py:24): odd extension of padlen samples, sosfilt_zi initial state scaled by the
 * first sample, forward pass, backward pass, trim.  The filter DESIGN (scipy.signal.butter,
 * sosfilt_zi; O(order) work) stays in the host layer; the O(n) recurrences run on the GPU.
 *   sos HOST f64[n_sections][6] (a0 == 1), zi HOST f64[n_sections][2] (= scipy.signal.sosfilt_zi(sos))
 *   x, y DEVICE f64[n];  work DEVICE f64[work_len], work_len >= par_sosfiltfilt_work_len(n, padlen)
 *   padlen = 3*(2*n_sections+1 - min(#(sos[:,2]==0), #(sos[:,5]==0)))  (scipy default), n > padlen.
 */
int64_t par_sosfiltfilt_work_len(int64_t n, int64_t padlen);
int par_sosfiltfilt_f64(int device, const double* sos, const double* zi, int n_sections, const double* x, int64_t n,
                        int64_t padlen, double* work, int64_t work_len, double* y, void* stream);

/* Batched form (r05): n_sig signals of ONE length n (signal i at x + i * x_stride, result at y + i * y_stride), n_filt = 1
 * (one cascade for all) or n_sig (cascade i for signal i: sos HOST f64[n_filt][n_sections][6], zi HOST f64[n_filt][n_sections][2]),
 * every stage ONE launch over the whole batch -- what dropouts_gui.process_heuristic does per band over the channels of a file
 * (dropouts_gui.py:314-321), or a multi-band analysis of one signal.  Each signal's result equals par_sosfiltfilt_f64's bit for
 * bit (same block / super-block chain).  padlen as above (the cascades of one call share it); n_sig <= 65535.
 * Synchronises the stream once (the parameter table's upload). */
int64_t par_sosfiltfilt_batch_work_len(int64_t n, int64_t padlen, int n_sig, int n_sections);
int par_sosfiltfilt_batch_f64(int device, const double* sos, const double* zi, int n_filt, int n_sections, const double* x,
                              int64_t x_stride, int n_sig, int64_t n, int64_t padlen, double* work, int64_t work_len, double* y,
                              int64_t y_stride, void* stream);

/* The block matrices both forms chain their 256-sample blocks with, for one section (HOST only, no device call; added at
 * ABI 109: par_version() stays 109).  section6 HOST f64[6] = (b0, b1, b2, a0, a1, a2); P4, Q4 HOST f64[4], row-major:
 * P = A^256, Q = A^65536 with A = [[-a1, 1], [-a2, 0]], each the exact power rounded to double (formed in double-double;
 * measured within one ulp of the largest entry, NOTES.md).  Exported so that the tests can pin them to the exact integer power. */
void par_sosfilt_block_matrices(const double* section6, double* P4, double* Q4);

/* ---- Spectral Expander (expander_gui.py) and time-averaged spectra (util/spectrum_flat.py), ABI 107 ------------------------ */
/* Band dB straight out of the STFT: out[f] (DEVICE f64[par_stft_frames(n, n_fft, hop)]) = mean over b in [bin_l, bin_u) of
 * 20 log10(|X_f[b]| / sqrt(n_fft) + 1e-7), the magnitude being the float32 value par_stft_f32 mode 1 writes and the log and
 * the sum float64 -- expander_gui.py:126-133 (nanmean of the band rows of spectrum_from_audio_stereo) without the
 * spectrogram.  Signal, window and frames as par_stft_f32 (x_stride: a channel of an interleaved file; reflect padding,
 * repeated for signals shorter than n_fft / 2).  n_fft*zeropad a power of two in [16, 16384], else PAR_ERR_UNSUPPORTED
 * (the host layer composes par_stft_big_f32 mode 1 and par_band_mean_db_f32 above); 0 <= bin_l < bin_u <= bins. */
int par_stft_band_db_f32(int device, const float* x, int64_t n, int64_t x_stride, int n_fft, int hop, int zeropad,
                         const float* window, int bin_l, int bin_u, double* out, void* stream);
/* acc[b] += sum over f < n_frames of 20 log10(mag[f * mag_pitch + b]) for b < bins (DEVICE f32 frame-major magnitudes as
 * par_stft_f32 mode 1 writes them; mag_pitch 0 = bins; DEVICE f64 acc[bins]).  Called once per frame chunk; the caller divides
 * by the total frame count (spectrum_flat.py:20-24 temporal mean).  Fixed summation order, no atomics. */
int par_mean_db_frames_f32(int device, const float* mag, int64_t n_frames, int64_t bins, int64_t mag_pitch, double* acc,
                           void* stream);
/* scipy.ndimage.uniform_filter1d(in[r], size, mode="nearest") for each of `rows` rows of n float64 (DEVICE, row-major,
 * out != in); size odd, any value (windows longer than the row repeat the edge values).  Compensated window sums: within
 * about an ulp of the exact window mean (expander_gui.py:134). */
int par_uniform_filter_nearest_f64(int device, const double* in, int64_t rows, int64_t n, int size, double* out, void* stream);
/* Expander gain (expander_gui.py:184-197), channel c < n_ch of the interleaved signal sig[i * sig_stride + c] (DEVICE f32):
 *   fac[j] = 10^((clip_upper - clip(curve[c * frames + j], clip_lower, clip_upper)) / 20)     (DEVICE f64 curve[n_ch][frames])
 *   g      = np.interp(i, j * hop, fac)   (end values held outside the frames)
 *   boosted = float64(sig) * g
 * out_f64 == NULL: out_f32[i * out_stride + c] = float32(boosted)  (the transition == 0 branch)
 * else:            out_f64[c * n + i] = boosted, out_f64[(n_ch + c) * n + i] = float64(sig)   (DEVICE f64[2][n_ch][n]: the
 *                  high-pass and low-pass inputs of the transition branch) */
int par_expand_gain_f32(int device, const float* sig, int64_t sig_stride, int n_ch, int64_t n, const double* curve,
                        int64_t frames, int hop, double clip_lower, double clip_upper, float* out_f32, int64_t out_stride,
                        double* out_f64, void* stream);
/* out[i * out_stride + c] = float32(a[c * n + i] + b[c * n + i])  (DEVICE; lp + hp of expander_gui.py:201, summed in float64) */
int par_sum_rows_f64_f32(int device, const double* a, const double* b, int n_ch, int64_t n, float* out, int64_t out_stride,
                         void* stream);
/* units.normalize (util/units.py:32-39) in place: d /= max|d| over d[0 .. count) (DEVICE f32), NaN propagating like np.max.
 * scratch: DEVICE, PAR_NORMALIZE_SCRATCH_BYTES.  Deterministic (max is order-free; the division is float32). */
#define PAR_NORMALIZE_SCRATCH_BYTES 4096
int par_normalize_f32(int device, float* d, int64_t count, void* scratch, void* stream);


/* ---- renoiser noise-floor gate (renoiser_gui.py:239-345), ABI 108 ------------------------------------------------------------ */
/* get_mask_fac + X * fac of renoiser_gui.py:273-278, 312-313 in place on a frame-major complex64 spectrogram (DEVICE
 * c64 spec[n_frames][pitch], the layout par_stft_f32 mode 0 and par_stft_big_f32 mode 0 write; pitch 0 = bins): bin b of every
 * frame passes unchanged when float32(hypot(re, im)) + 1e-7f >= cutoff[b] (DEVICE f32[bins]), else both parts are multiplied
 * by `low` (float32(10^(gain/20))) as numpy multiplies complex64 by float32.  |X| is the float32 value numpy's np.abs gives
 * for complex64 (its SIMD loop: larger * sqrt(fma(r, r, 1)), r = smaller / larger); the cutoffs come from the float64
 * thresholds through renoiser.gate_cutoffs (a NaN cutoff gates the bin).  The result equals numpy's on the same spectrum bit
 * for bit. */
int par_gate_spectrum_f32(int device, float* spec, int64_t n_frames, int64_t bins, int64_t pitch, const float* cutoff, float low,
                          void* stream);
/* Fused renoiser apply (renoiser_gui.py:296-319), one launch for n_ch channels: channel c < n_ch of the interleaved signal
 * x[i * x_stride + c] (DEVICE f32, i < n) is zero-extended to n + n_fft/2 (fix_length), transformed (blackmanharris or any
 * `window`, DEVICE f32[n_fft]; reflect padding of the extended length, frames and scaling of par_stft_f32 mode 0), gated as
 * par_gate_spectrum_f32 does, inverse transformed and overlap-added with the window-sum-square normalisation of
 * par_istft_f32 (length n), and written to y[i * y_stride + c] (DEVICE f32).  No spectrogram reaches HBM.  n_fft a power of
 * two in [16, 8192] and 1 <= hop <= n_fft, else PAR_ERR_UNSUPPORTED (compose par_stft_*, par_gate_spectrum_f32 and
 * par_istft_f32).  Bins hold the same gate decisions as par_gate_spectrum_f32 on par_stft_f32's spectrum. */
int par_gate_stft_f32(int device, const float* x, int64_t n, int64_t x_stride, int n_ch, int n_fft, int hop, const float* window,
                      const float* cutoff, float low, float* y, int64_t y_stride, void* stream);
/* Frames par_gate_stft_f32 transforms per channel (each forward and back; host only, for reporting the streaming form's
 * redundant-frame share); 0 when the size is unsupported. */
int64_t par_gate_stft_transformed_frames(int64_t n, int n_fft, int hop);
/* acc[b] += sum over f < n_frames of mag[f * mag_pitch + b] (float64, the fixed order of par_mean_db_frames_f32): the
 * numerator of the selection profile np.average(mag[:, f0:f1], axis=1) (renoiser_gui.py:340). */
int par_mean_mag_frames_f32(int device, const float* mag, int64_t n_frames, int64_t bins, int64_t mag_pitch, double* acc,
                            void* stream);

/* ---- harmonic / percussive separation (util/decompose.py, experiments/hpss_gui.py), ABI 109 ---------------------------------- */
/* decompose.hpss on a frame-major spectrogram (DEVICE spec[n_frames][pitch], pitch 0 = bins; is_complex != 0: complex64, the
 * layout par_stft_f32 mode 0 and par_stft_big_f32 mode 0 write, else float32 magnitudes, read through fabs).  Per bin:
 *   harm = scipy.ndimage.median_filter(|S|, win_harm, mode="reflect") along frames, perc = the same over win_perc along bins
 *          (window offsets -(k/2) .. k-1-k/2, the element of rank k/2, half-sample symmetric reflection repeated as often as
 *          the axis needs; 1 <= k <= PAR_HPSS_MAX_KERNEL, odd or even).  |S| is numpy's complex64 np.abs (see
 *          par_gate_spectrum_f32, without its + 1e-7): the medians are selections and equal scipy's on np.abs(spec) bit for bit.
 *          A NaN magnitude ranks above inf in a window (np.sort's order): a median is NaN when the element of rank k/2 is.
 *   mask_h = softmask(harm, perc * margin_h), mask_p = softmask(perc, harm * margin_p) in float32: Z = max(X, Xref);
 *          Z < FLT_MIN -> 0.5 when both margins are 1, else 0; else (X/Z)^power / ((X/Z)^power + (Xref/Z)^power) (power 2
 *          squares, 1 and 0.5 are exact too); power = +inf: the hard mask X > Xref.  The masks propagate NaN as numpy does
 *          (np.maximum keeps it): a NaN in X or Xref gives a NaN mask for every finite power, and 0 from the hard mask.
 * out_kind PAR_HPSS_COMPONENTS: out_h = S * mask_h, out_p = S * mask_p (the input's type);  PAR_HPSS_MASKS: the two float32 masks;
 * PAR_HPSS_HARMONIC: out_h = S * mask_h only (out_p may be NULL; decompose.harmonic);  PAR_HPSS_MEDIANS: float32 harm and perc.
 * S * mask is numpy's product: for complex64 the complex product with mask + 0i, so an infinite or NaN part of S makes both
 * parts of the result NaN and a zero result has numpy's sign; finite non-zero parts are scaled one by one.
 * Outputs are DEVICE [n_frames][pitch] arrays of their element type and must not overlap spec or each other.  No scratch.
 * Kernel sizes outside 1..99, power <= 0 (or NaN), a margin below 1 and null pointers: PAR_ERR_ARG before any device call. */
#define PAR_HPSS_MAX_KERNEL 99
#define PAR_HPSS_COMPONENTS 0
#define PAR_HPSS_MASKS 1
#define PAR_HPSS_HARMONIC 2
#define PAR_HPSS_MEDIANS 3
int par_hpss_f32(int device, const void* spec, int is_complex, int64_t n_frames, int64_t bins, int64_t pitch, int win_harm,
                 int win_perc, double power, double margin_h, double margin_p, void* out_h, void* out_p, int out_kind, void* stream);
/* r[i * r_stride] = x[i * x_stride] - (h[i * h_stride] + p[i * p_stride]), i < n, float32 (DEVICE; the residual of
 * hpss_gui.py:145 on channel views of interleaved signals). */
int par_residual_f32(int device, const float* x, int64_t x_stride, const float* h, int64_t h_stride, const float* p,
                     int64_t p_stride, int64_t n, float* r, int64_t r_stride, void* stream);

/* ---- fixed-ratio resampling (resampy.resample(x, sr_orig, sr_new, axis=0, filter='sinc_window', num_zeros=Z)) --------------------
 * par_resample_fixed_out_len and par_resample_fixed_f32 are added at ABI 109: par_version() stays 109. */
/* Samples the resampler writes for n input samples: int(n * sr_new / sr_orig), evaluated left to right in double (host only;
 * -1 for a negative n or rates that are not finite and positive). */
int64_t par_resample_fixed_out_len(int64_t n, double sr_orig, double sr_new);
/* y[t * y_stride], t < n_out, = Smith's band-limited interpolation of x[i * x_stride], i < n (DEVICE f32, channel views of
 * interleaved arrays; x and y distinct buffers) at the positions t * (1 / ratio), ratio = sr_new / sr_orig, over resampy
 * 0.4's interpolated 'sinc_window' table: 512 entries per zero crossing, rolloff 0.945, symmetric Hann taper, linear
 * interpolation between entries, table step int(min(1, ratio) * 512), the sum scaled by ratio when ratio < 1.  Positions,
 * table offsets and interpolation fractions are float64 and equal numpy's bit for bit; weights and sums are float32.  The
 * wings are cut at the signal's ends (no padding): nothing outside x[0, n) is read, no other cell of y is written.
 * n_out must be par_resample_fixed_out_len(n, sr_orig, sr_new).  Null pointers, rates that are not finite and positive,
 * num_zeros outside 1..64, strides < 1, a wrong n_out and x == y: PAR_ERR_ARG before any device call; n == 0 or n_out == 0:
 * PAR_OK, nothing done; ratio outside [1/16, 16]: PAR_ERR_UNSUPPORTED.  The table is built once per (device, num_zeros). */
int par_resample_fixed_f32(int device, const float* x, int64_t n, int64_t x_stride, double sr_orig, double sr_new, int num_zeros,
                           float* y, int64_t n_out, int64_t y_stride, void* stream);
/* ---- renoiser "Gauge offset" (renoiser_gui.py:347-369 sniff_offset, experiments/renoiser.py:59-73) -----------------------------
 * par_gauge_frames, par_gauge_scratch_bytes and par_gauge_offset_f32 are added at ABI 109: par_version() stays 109. */
/* Frames of the reference's STFT for pad `offset`: with M = n + offset + n_fft/2 samples, reflect-padded by n_fft/2 at both
 * ends, (M + 2 (n_fft/2) - n_fft) / hop + 1 -- for an even n_fft (n + offset + n_fft/2) / hop + 1 (host only; -1 for n < 0,
 * n_fft < 2, hop < 1 or a negative offset). */
int64_t par_gauge_frames(int64_t n, int n_fft, int hop, int offset);
/* Bytes of DEVICE scratch par_gauge_offset_f32 needs (host only; 0 for arguments it refuses): three float64 sums per dense
 * workgroup and residue slot, and one complex64 per pad and edge frame. */
size_t par_gauge_scratch_bytes(int64_t n, int n_fft, int hop);
/* stds[i], i < hop (DEVICE f64) = the standard deviation over the frames (numpy's std of a complex array, ddof 0) of
 *   z(i, j) = sum_m p_i[j hop + m] (h_re[m] + 1j h_im[m]),   m = 0 .. n_fft - 1,   j < par_gauge_frames(n, n_fft, hop, i)
 * where p_i is x[k * x_stride], k < n (DEVICE f32, a channel view of an interleaved signal) with i zeros in front, zero-extended
 * by n_fft/2 and reflect-padded by n_fft/2 at both ends as par_stft_f32 pads: with M = n + i + n_fft/2, padded index q maps to
 * r = q - n_fft/2, r < 0 to -r, r >= M to 2 (M - 1) - r, value x[r - i] for i <= r < i + n, else 0.  With h (DEVICE f32
 * [n_fft] each part) = renoiser.gauge_filter, z is the mean of bins l..u-1 of the reference's STFT and stds its curve.  Each
 * part of z is one float32 FMA chain over ascending m; sum z, sum |z|^2 are float64 in a fixed order (no atomics: two runs are
 * bit-identical); std = sqrt(max(0, sum|z|^2 / F - |sum z / F|^2)), NaN kept.  Any n_fft >= 2 and hop >= 1.  Nothing but
 * stds[0 .. hop) and scratch is written.  Null pointers, n < 1, n_fft < 2, hop < 1, x_stride < 1, scratch_bytes below
 * par_gauge_scratch_bytes (or a scratch that is not 8-byte aligned): PAR_ERR_ARG before any device call. */
int par_gauge_offset_f32(int device, const float* x, int64_t n, int64_t x_stride, int n_fft, int hop, const float* h_re,
                         const float* h_im, double* stds, void* scratch, size_t scratch_bytes, void* stream);
/* ---- dynamics matcher (experiments/decompressor_cmd.py:26-188 process, after its band-pass) -----------------------------------
 * par_windowed_rms_log10_f64, par_level_match_f64, par_uniform_filter_reflect_f64, par_dynamics_factor_f64 and
 * par_dynamics_apply_f32 are added at ABI 109: par_version() stays 109.  All work on the caller's stream, none synchronises the
 * host, none needs scratch; fixed summation orders, no atomics: two runs are bit-identical. */
/* out[r * F + j], j < F = ceil(n / hop) (DEVICE f64) = the windowed RMS of decompressor_cmd.py:16-23 of row r of x (DEVICE
 * f64[rows][x_pitch], n samples used):
 *   rms = sqrt(sum of x[i]^2 over j hop <= i < min(j hop + sz, n), divided by the number of those samples)
 * -- the last windows are truncated and their mean divides by the truncated length -- then np.clip(rms, floor, None) (a NaN
 * stays) and, for log10_out != 0, log10 of it (:93-96 with floor 0.0005; a clipped frame stores the host libm's log10(floor));
 * log10_out == 0 stores the clipped RMS itself (floor 0: the plain RMS, exactly 0 for a silent window).  Any hop >= 1 and sz >= 1 (sz % hop != 0, sz < hop, sz > n).  Squares and
 * sums are float64: per hop-aligned piece a fixed order over the lanes, then the pieces of a frame ascending; at most sz + 1
 * roundings bear on a sum.  Every sample is read once per 1024 frames (+ sz samples).  Null pointers, rows outside 1..65535,
 * n, hop or sz < 1, x_pitch < n, a NaN floor: PAR_ERR_ARG before any device call. */
int par_windowed_rms_log10_f64(int device, const double* x, int64_t x_pitch, int64_t rows, int64_t n, int hop, int sz, double floor,
                               int log10_out, double* out, void* stream);
/* out_b[r * F + j] = (b[r * F + j] - mean(b[r])) + mean(a[r]), r < rows, j < F (DEVICE f64; decompressor_cmd.py:97, in its
 * order).  Each mean is a float64 sum in a fixed two-level order (1024 strided runs, ascending, then a tree over them) divided
 * by F.  out_b may be b itself, not a.  Null pointers, rows or F < 1: PAR_ERR_ARG before any device call. */
int par_level_match_f64(int device, const double* a, const double* b, int64_t rows, int64_t F, double* out_b, void* stream);
/* scipy.ndimage.uniform_filter1d(in[r], size) -- the default mode "reflect" (d c b a | a b c d | d c b a), origin 0 -- for each
 * of `rows` rows of n float64 (DEVICE, row-major, out != in): out[i] = mean of the extended row over
 * [i - size / 2, i + size - size / 2 - 1]; size >= 1 of either parity, rows shorter than the window reflect repeatedly
 * (position q reads m = q mod 2n, or 2n - 1 - m for m >= n).  Compensated window sums as par_uniform_filter_nearest_f64:
 * within about an ulp of the exact window mean; size 1 returns the input bit for bit (decompressor_cmd.py:99-100). */
int par_uniform_filter_reflect_f64(int device, const double* in, int64_t rows, int64_t n, int size, double* out, void* stream);
/* Steps :109-166 for rows r < rows of F frames (DEVICE f64 a = the source's smoothed log curve, b = the reference's), with
 * ch = corr_sz / 2, K = (F - 1) / ch, k = i / ch + 1, m = i % ch and hann (DEVICE f64[corr_sz]) = np.hanning(corr_sz), computed
 * by the host (no cosine is evaluated on the device):
 *   aligned[i] = 0.0 (+ a[i] * hann[m + ch] if k <= K) (+ a[i] * hann[m] if k + 1 <= K)     two products, added in this order
 *   fac[i]     = nan_to_num(clip(10^b[i] / 10^aligned[i], 0, 2))                               a NaN becomes 0
 * which is the reference's Hann overlap-add of the edge-padded curve with do_sync False, bit for bit -- including its tail:
 * frames from (K - 1) ch on carry the falling half of the window only, frames from K ch - 1 on (all of them for F <= ch) are 0,
 * so fac = min(10^b, 2) there.  aligned_or_null: when not NULL, receives aligned (f64[rows][F]).  corr_sz odd or < 2, null
 * pointers, rows outside 1..65535, F < 1: PAR_ERR_ARG before any device call. */
int par_dynamics_factor_f64(int device, const double* a, const double* b, int64_t rows, int64_t F, const double* hann, int corr_sz,
                            double* aligned_or_null, double* fac, void* stream);
/* Steps :169-185 on the interleaved signal sig[i * sig_stride + c], c < n_ch, i < n (DEVICE f32) with fac (DEVICE
 * f64[n_ch][F], F = ceil(n / hop), frame j at sample j hop):
 *   g_c  = np.interp(i, j hop, fac[c]): fac[c][j] on a key, (fac[c][j+1] - fac[c][j]) / hop * (i - j hop) + fac[c][j] between
 *          two, fac[c][F-1] from the last key on
 *   g    = np.mean over the channels: the left-to-right sum g_0 + g_1 + .. divided by n_ch
 *   out[i * out_stride + c] = float32(float64(sig) * g)        one rounding to float32
 * Equals numpy on the same fac bit for bit.  n_ch > 8: PAR_ERR_UNSUPPORTED.  Null pointers, n, hop or n_ch < 1, a stride below
 * n_ch, F != ceil(n / hop), out == sig: PAR_ERR_ARG before any device call. */
int par_dynamics_apply_f32(int device, const float* sig, int64_t sig_stride, int n_ch, int64_t n, const double* fac, int64_t F,
                           int hop, float* out, int64_t out_stride, void* stream);
/* ---- stereo balance (pypan_gui.py:53-58 run_resample, :78-104 the Shift branch of on_mouse_release) ------------------------------
 * par_pan_ratio_scratch_bytes, par_pan_ratio_f32, par_stft_pan_scratch_bytes, par_stft_pan_ratio_f32 and par_pan_apply_f32 are
 * added at ABI 109: par_version() stays 109.  All work on the caller's stream and none synchronises the host.
 *
 * A box is four int32 (bin_l, bin_u, frame_0, frame_1), half-open: the integers the reference derives at :81-98 (the host layer's
 * pypan.box_to_cells).  `boxes` is DEVICE int32[n_box][4], read by the kernels; `boxes_host` is a HOST copy of the same numbers,
 * from which the call validates every box, sizes its launches and checks the scratch before any device call (as
 * par_gather_windows_f64 takes its geometry twice).  A box whose bin range leaves [0, bins] or whose frame range leaves
 * [0, n_frames] is PAR_ERR_ARG (the host layer clamps as the reference does); an empty range inside those limits is legal.
 * 1 <= n_box <= 65535; at most 2^31 - 1 (box, frame) pairs per call. */
/* Bytes of DEVICE scratch for these boxes (host only; 0 for a null pointer or n_box outside 1..65535): int64[n_box + 1] offsets,
 * padded to 16 bytes, and one (float64 sum, int64 count) pair per frame of every box that holds a cell. */
size_t par_pan_ratio_scratch_bytes(const int32_t* boxes_host, int64_t n_box);
/* fac[b] (DEVICE f64) = np.nanmean(L[bin_l:bin_u, frame_0:frame_1] / R[...]) and count[b] (DEVICE int64) = the cells that entered
 * it, for box b < n_box of two FRAME-MAJOR float32 magnitude spectrograms magL, magR [n_frames][pitch] (DEVICE; what par_stft_f32
 * and par_stft_big_f32 write in mode 1; pitch 0 = bins).  q = float32(L / R) is the correctly rounded float32 quotient; the cells
 * whose q is not NaN are summed in float64 and counted, a +-inf quotient included, as numpy does; fac = sum / count, NaN when
 * count == 0 (an empty box, which is how nanmean treats an empty slice, or a box of NaN cells only).  The order of the sum is
 * fixed -- a frame's cells over 64 lanes and a xor tree, the frames of a box in 256 ascending strided runs, a xor tree and four
 * partials in order -- and no atomics are used: two runs are bit-identical.  Nothing but fac[0 .. n_box), count[0 .. n_box) and
 * scratch is written.  Null pointers, sizes < 1, pitch < bins, a scratch that is not 16-byte aligned, a box outside the
 * spectrogram: PAR_ERR_ARG; scratch_bytes below par_pan_ratio_scratch_bytes: PAR_ERR_WORKSPACE; all before any device call. */
int par_pan_ratio_f32(int device, const float* magL, const float* magR, int64_t n_frames, int64_t bins, int64_t pitch,
                      const int32_t* boxes, const int32_t* boxes_host, int64_t n_box, double* fac, int64_t* count, void* scratch,
                      size_t scratch_bytes, void* stream);
/* The same fac and count straight from the two channels: xL, xR (DEVICE f32, n samples each at the common element stride x_stride;
 * an interleaved stereo file is xR == xL + 1 with x_stride == 2, whose samples then arrive as one 8-byte load per L/R pair;
 * planar channels and wider strides work too).  Padding, framing, scaling and the float32 magnitude are those of par_stft_f32 mode
 * 1 on each channel, bins = n_fft*zeropad/2 + 1 and n_frames = par_stft_frames(n, n_fft, hop); only frames inside a box are
 * transformed (a frame inside k boxes k times), and no spectrogram is stored.  The quotients, their float64 sums per (box, frame)
 * and the reduction over a box's frames are par_pan_ratio_f32's, the order inside a frame differs (the lanes own bins as the
 * transform leaves them).  Bit-identical from run to run.  n_fft*zeropad must be a power of two in [16, 16384], otherwise
 * PAR_ERR_UNSUPPORTED (compose par_stft_big_f32 mode 1 twice and par_pan_ratio_f32).  Errors as par_pan_ratio_f32.
 * par_stft_pan_scratch_bytes == par_pan_ratio_scratch_bytes (one layout). */
size_t par_stft_pan_scratch_bytes(const int32_t* boxes_host, int64_t n_box);
int par_stft_pan_ratio_f32(int device, const float* xL, const float* xR, int64_t x_stride, int64_t n, int n_fft, int hop, int zeropad,
                           const float* window, const int32_t* boxes, const int32_t* boxes_host, int64_t n_box, double* fac,
                           int64_t* count, void* scratch, size_t scratch_bytes, void* stream);
/* out[i * out_stride] = float32(float64(sig[i * sig_stride]) * np.interp(i, xp, fp)), i < n (DEVICE f32 in and out, channel views
 * of interleaved arrays; xp, fp DEVICE f64[m], xp non-decreasing): run_resample's `signal[:, 1] * af` as the FLOAT file stores it.
 * np.interp's arithmetic is restated operation by operation (the interpolation step of par_lag_to_pos_f64): equal to numpy bit for
 * bit, fp[0] before the first knot and fp[m-1] behind the last, fp[j] exactly on a knot (the last of equal knots), NaN and inf in
 * fp or sig propagating as numpy's.  m == 1 is a constant gain.  n == 0: PAR_OK, nothing done.  Null pointers, m < 1 (np.interp
 * raises ValueError), n < 0, a stride < 1: PAR_ERR_ARG before any device call. */
int par_pan_apply_f32(int device, const float* sig, int64_t sig_stride, int64_t n, const double* xp, const double* fp, int64_t m,
                      float* out, int64_t out_stride, void* stream);
/* ---- Differential EQ (difeq_gui.py:24-38 get_eq): time-averaged dB spectra straight from the samples ---------------------------
 * par_stft_mean_db_scratch_bytes and par_stft_mean_db_f32 are added at ABI 109: par_version() stays 109.
 *
 * mean[c][b] (DEVICE f64[n_ch][bins], bins = n_fft*zeropad/2 + 1) = (sum over frames f of 20 log10((double) m_f[b])) / n_frames
 * for every channel c < n_ch of the interleaved signal x[i * x_stride + c] (DEVICE f32, n samples per channel), where m_f[b] is
 * the float32 magnitude par_stft_f32 mode 1 writes for that channel (padding, framing, scaling and the repeated reflection of a
 * signal shorter than n_fft/2 included) and n_frames = par_stft_frames(n, n_fft, hop): np.mean(to_dB(get_mag(x)), axis=1) of
 * util/spectrum_flat.py:20-24 in float64, for all channels in one launch and with no spectrogram stored.
 * Order of the sum (fixed by the arguments alone, no atomics, bit-identical from run to run and from device to device): the
 * frames are cut into runs of R = max(16, ceil(n_frames / 512)) consecutive frames; inside a run the terms of a bin are added in
 * float64 in ascending frame order starting from 0; the runs' partial sums are added in ascending run order starting from run
 * 0's; the total is divided by n_frames once.  `scratch` (DEVICE, 8-byte aligned, par_stft_mean_db_scratch_bytes: one float64 row of
 * bins per run and channel) needs no initialisation; nothing but mean[0 .. n_ch*bins) and scratch is written.  The work runs on
 * the caller's stream without host synchronisation.  n_fft*zeropad must be a power of two in [16, 16384] (n_fft even), otherwise
 * PAR_ERR_UNSUPPORTED (compose par_stft_big_f32 mode 1 and par_mean_db_frames_f32).  Null pointers, n, hop, zeropad < 1,
 * n_fft < 2, n_ch outside 1..8, x_stride < n_ch, misaligned mean or scratch: PAR_ERR_ARG; scratch_bytes too small:
 * PAR_ERR_WORKSPACE; all before any device call. */
/* Bytes of DEVICE scratch (host arithmetic; 0 for sizes par_stft_mean_db_f32 does not take) */
size_t par_stft_mean_db_scratch_bytes(int64_t n, int n_fft, int hop, int zeropad, int n_ch);
int par_stft_mean_db_f32(int device, const float* x, int64_t n, int64_t x_stride, int n_ch, int n_fft, int hop, int zeropad,
                         const float* window, double* mean, void* scratch, size_t scratch_bytes, void* stream);
/* ---- Cyclic wow (experiments/cyclic_wow.py): pilot-tone track straight from the samples, fold at candidate cycle lengths -------
 * par_stft_track_peak_f64 and par_cycle_fold_f64 are added at ABI 109: par_version() stays 109.
 *
 * par_stft_track_peak_f64: freqs[i] (DEVICE f64[count]; in = the sampled trail, out = the traced frequency in Hz) for the frames
 * frame_0 + i, i < count, of the signal x[k * x_stride] (DEVICE f32, n samples): what par_track_peak_f64 writes for the same
 * frame_0 / count / freqs / sr / tolerance_oct / mode on the spectrogram par_stft_f32 mode 1 stores for x, bit for bit, without
 * the spectrogram.  Every value the tracker compares is the float32 magnitude m_f[b] of that spectrogram (padding, framing,
 * scaling and the repeated reflection of a signal shorter than n_fft/2 included) for db = 0, and for db = 1 its float32 dB,
 * (float)(20 log10((double) m_f[b])) with the float64 logarithm of par_band_mean_db_f32 (|error| <= 1e-15 against numpy's log10):
 * the float32 dB spectrogram experiments/cyclic_wow.py:34-37 hands PeakTracker.  Per frame: the band [NL, NU) of
 * par_track_peak_f64 (mode 0: around freqs[i]; mode 1: around freqs[0], read before the launch, the tolerance halved for i > 2),
 * the first maximum of the band (a NaN never wins; a NaN on bin NL keeps bin NL), is_peak on its two neighbours (bin 0 reads bin
 * bins - 1 as its left one), parabolic() in float64, bin / (n_fft*zeropad) * sr.  No sum is formed: the result does not depend on
 * the launch shape and is bit-identical from run to run.  status (DEVICE int32) and its errors are par_track_peak_f64's: an empty
 * band PAR_ERR_EMPTY_BAND (that frame's freqs entry is left as it was), a peak on the last bin PAR_ERR_INDEX, a band past the last
 * bin PAR_ERR_SHAPE; these come from a completed launch.  Nothing but freqs[0 .. count) and status is written.  Synchronises (it
 * returns the status).  count == 0: PAR_OK, nothing done.  n_fft*zeropad must be a power of two in [16, 16384] (n_fft even),
 * otherwise PAR_ERR_UNSUPPORTED (compose par_stft_big_f32 mode 1 and par_track_peak_f64).  Null pointers, n, hop, zeropad or
 * x_stride < 1, n_fft < 2, count < 0, frame_0 < 0, frame_0 + count > par_stft_frames(n, n_fft, hop), mode or db outside 0..1:
 * PAR_ERR_ARG; all argument errors before any device call. */
int par_stft_track_peak_f64(int device, const float* x, int64_t n, int64_t x_stride, int n_fft, int hop, int zeropad,
                            const float* window, int64_t frame_0, int64_t count, double* freqs, double sr,
                            double tolerance_oct, int mode, int db, int32_t* status, void* stream);
/* par_cycle_fold_f64: for every candidate cycle length P = p_first + c, c < n_cand, the track v (DEVICE f64[count]) is cut into
 * V = count / P whole views (integer division; the frames behind V * P are dropped) and averaged over the views:
 *   avg[c * avg_pitch + p] = (v[p] + v[P + p] + ... + v[(V - 1) P + p]) / V,  p < P
 * the sum in float64 in ascending view order starting from view 0, then one division: np.mean(np.split(v[:V * P], V), axis=0)
 * of get_avg (experiments/cyclic_wow.py:9-27), equal to numpy bit for bit for P >= 2 (numpy reduces the outer axis of a
 * C-contiguous array row after row).  At P == 1 numpy folds the (V, 1) array into one contiguous run and sums it pairwise; the
 * order here stays as stated and the two differ by at most 2 (V - 1) 2^-53 sum|v| / V.  delta[c] (DEVICE f64[n_cand]) = max_p avg - min_p avg; a NaN in a row makes its delta NaN, as np.max /
 * np.min propagate it.  avg (DEVICE f64) may be null; otherwise only avg[c * avg_pitch + 0 .. P) is written, avg_pitch >=
 * p_first + n_cand - 1.  No atomics: bit-identical from run to run.  The work runs on the caller's stream without host
 * synchronisation.  Null v or delta, p_first < 1, n_cand < 1, count < 0, p_first + n_cand - 1 > count (the reference's np.split
 * into zero sections raises), avg_pitch below the longest cycle: PAR_ERR_ARG before any device call. */
int par_cycle_fold_f64(int device, const double* v, int64_t count, int p_first, int n_cand, double* avg, int64_t avg_pitch,
                       double* delta, void* stream);
/* ---- MaxMono dropout repair (dropouts_gui.py:137-163): per STFT bin the louder (max) or the quieter (min) of two channels --------
 * par_select_spectrum_f32, par_maxmono_stft_f32, par_maxmono_stft_supported and par_maxmono_stft_transformed_frames are added at
 * ABI 109: par_version() stays 109.  All work on the caller's stream, none synchronises the host.
 *
 * par_select_spectrum_f32: specL, specR (DEVICE c64 [n_frames][pitch], the layout par_stft_f32 mode 0 writes; pitch 0 = bins) ->
 *   out_max = where(|L| > |R|, L, R), out_min = where(|L| < |R|, L, R), same layout, padding cells untouched.
 * |.| is the float32 value numpy's np.abs gives for complex64 (see par_gate_spectrum_f32).  On a tie both outputs take R, and
 * where a magnitude is NaN both comparisons are false, so again both take R.  The result is the selected input's bits: nothing
 * is multiplied, so NaN payloads, -0.0 and denormals pass through, and it equals numpy's np.where on the same spectra bit for
 * bit.  Either output may be NULL (not both).  Outputs must not overlap the inputs or each other.  Null inputs, both outputs
 * NULL, n_frames < 0, bins < 1, pitch < bins, overlapping ranges: PAR_ERR_ARG before any device call.  n_frames == 0: PAR_OK. */
int par_select_spectrum_f32(int device, const float* specL, const float* specR, int64_t n_frames, int64_t bins, int64_t pitch,
                            float* out_max, float* out_min, void* stream);
/* Fused MaxMono, one launch: the channel views xL[i * x_stride] and xR[i * x_stride] (DEVICE f32, i < n; the two columns of an
 * interleaved file for instance) are each zero-extended to n + n_fft/2 (fix_length) and transformed (`window` DEVICE f32[n_fft];
 * reflect padding of the extended length, frames and scaling of par_stft_f32 mode 0), selected bin by bin as
 * par_select_spectrum_f32 does, and the max and the min spectrum are inverse transformed and overlap-added with the
 * window-sum-square normalisation of par_istft_f32 (length n) into y_max[i * ymax_stride] and y_min[i * ymin_stride] (DEVICE f32).
 * No spectrogram reaches HBM.  y_max or y_min may be NULL (not both); that inverse is then skipped.  Contract: bin k
 * holds the decision par_select_spectrum_f32 makes on par_stft_f32's spectra of the two channels, except that it may hold
 * either channel where the two magnitudes differ by no more than 2^-21 (|L[k]| + |L[H-k]| + |R[k]| + |R[H-k]|), H = n_fft/2
 * (16 float32 ulps where the four are alike): a last-bit change of the packed transform's cells k and H - k moves a bin by
 * up to 2^-22 of that sum.  tests/test_maxmono_gpu.py holds the kernel to this.  The forward path is K_stft
 * mode 0's, operation by operation in the source, but the compiler contracts one complex multiply of the last transform stage
 * into a different fused multiply-add in the two kernels, so a part of a bin can differ from par_stft_f32's in its last
 * bit.  Measured: 2 bins of 2.1e8 on a 10-min stereo file at 2048/128 decided differently (5.3e-5 of the peak over one
 * frame's reach each), none at 512/64 and 2048/512 (NOTES.md, MaxMono).  Ties by construction (xR = -xL, xR = xL) are exact in
 * both.  Fused sizes: n_fft a power of two in
 * [16, 8192] and 1 <= hop <= n_fft, as far as the frames, two overlap-add rings of n_fft + Frames * hop floats (Frames =
 * max(1, 4096 / n_fft) frames per round) and hop floats of window sums fit 160 KB of LDS: every hop up to n_fft = 4096, and
 * hop <= 5114 at n_fft = 8192 (par_maxmono_stft_supported says so without a device).  Everything else returns
 * PAR_ERR_UNSUPPORTED with the outputs untouched (compose par_stft_f32, par_select_spectrum_f32 and par_istft_f32).  Null
 * pointers, n < 1, hop < 1, a stride < 1: PAR_ERR_ARG; all before any device call. */
int par_maxmono_stft_f32(int device, const float* xL, const float* xR, int64_t n, int64_t x_stride, int n_fft, int hop,
                         const float* window, float* y_max, int64_t ymax_stride, float* y_min, int64_t ymin_stride, void* stream);
/* 1 when par_maxmono_stft_f32 takes (n_fft, hop), else 0 (host arithmetic) */
int par_maxmono_stft_supported(int n_fft, int hop);
/* Frames par_maxmono_stft_f32 transforms per channel (host only, for reporting the streaming form's redundant-frame share);
 * 0 when the size is unsupported. */
int64_t par_maxmono_stft_transformed_frames(int64_t n, int n_fft, int hop);
/* ---- Zero-crossing flutter analysis (experiments/zerocrossing_wow.py:17-30, util/wow_detection.py:342-358) ------------------------
 * par_crossing_smooth_f64 and par_interp_f64 are added at ABI 109: par_version() stays 109.  Both work on the caller's stream and
 * neither synchronises the host.
 *
 * par_crossing_smooth_f64: crossings (DEVICE int64[c], strictly ascending: what par_zero_crossings_f64 compacts) -> n = c - 1
 * values per output.  With d[i] = (float)(crossings[i + 1] - crossings[i]) (the difference in int64, one rounding to float32:
 * np.diff(crossings).astype(np.float32)) and kernel (DEVICE f64[span]; the host's scipy.signal.get_window("hann", span) / span * 2,
 * no cosine is computed on the device):
 *   smooth[i] = sum_{j < span} (double)P[i + span + (span - 1) / 2 - j] * kernel[j]
 *               P = np.pad(d, span, mode="reflect"), taken in closed form: q = index - span, k = q mod 2 (n - 1) (non-negative),
 *               k >= n -> 2 (n - 1) - k, P[index] = d[k]; numpy's reflection for every pad width, wider than the array included.
 *               This is np.convolve(P, kernel, mode="same")[span:-span].  Products and sums are float64, every rounding separate.
 *               Summation order (fixed, the same in every run and for every launch): four partial sums over the taps j = 0, 1, 2,
 *               3 (mod 4), each in ascending j, the up to three tail taps j >= span - span % 4 added to partial sums 0, 1, 2 in
 *               turn, then (s0 + s1) + (s2 + s3).  Every term is non-negative, so |smooth - exact| <= (span + 2) 2^-53 exact.
 *   freq[i]   = (sr / 2) / smooth[i]                  float64, one division
 *   xp[i]     = (double)crossings[i] / sr + t0        two roundings: numpy's crossings[:n] / sr + t0
 *   raw[i]    = (float)(sr / 2) / d[i]                one float32 division: the reference's "raw" curve
 * smooth (DEVICE f64[n]) and raw (DEVICE f32[n]) may be NULL; freq and xp are DEVICE f64[n].  span in
 * [1, PAR_CROSSING_SMOOTH_MAX_SPAN]: the periods a workgroup needs and the weights sit in LDS.  At span 1 the one weight is 2
 * and smooth = 2 d: the reference's own result there, kept.  Null crossings / kernel / freq / xp, c < 3, span outside that range,
 * sr not finite or not positive: PAR_ERR_ARG before any device call, nothing written. */
#define PAR_CROSSING_SMOOTH_MAX_SPAN 4096
int par_crossing_smooth_f64(int device, const int64_t* crossings, int64_t c, const double* kernel, int span, double sr, double t0,
                            double* smooth, double* freq, double* xp, float* raw, void* stream);
/* par_interp_f64: out[k] = np.interp(x[k], xp, fp), k < nx (x, out DEVICE f64[nx]; xp non-decreasing, fp: DEVICE f64[m]), numpy's
 * arithmetic restated operation by operation (slope = (fp[j+1] - fp[j]) / (xp[j+1] - xp[j]); slope * (x - xp[j]) + fp[j], no fused
 * multiply-add): equal to numpy bit for bit.  fp[0] below xp[0], fp[m-1] above xp[m-1]; on equal knots fp at the last of them;
 * NaN and inf in fp propagate as numpy's; a NaN abscissa gives NaN (with one knot fp[0], as numpy).  x in any order.  nx == 0:
 * PAR_OK, nothing done.  m < 1, nx < 0, null pointers: PAR_ERR_ARG before any device call. */
int par_interp_f64(int device, const double* x, int64_t nx, const double* xp, const double* fp, int64_t m, double* out,
                   void* stream);
/* ---- Spectrogram image (util/spectrum.py: Spectrum.update_data, SpectrumCanvas.compute_spectra, set_clims / set_cmap) -------------
 * par_stft_peak_image_scratch_bytes, par_stft_peak_image_f32, par_peak_image_f32 and par_image_colorize_u8 are added at ABI 109:
 * par_version() stays 109.  All work on the caller's stream and none synchronises the host.
 *
 * The picture is a PEAK-HOLD reduction of the float32 magnitude spectrogram to width x height cells.  Column c is the half-open
 * frame range cols[c] = (lo, hi) (int64[width][2]), row r the half-open bin range rows[r] = (lo, hi) (int32[height][2]); the host
 * layer's spectrogram.geometry derives both.  `cols` / `rows` are DEVICE arrays the kernels read, `cols_host` / `rows_host` HOST
 * copies of the same numbers from which the call validates the tables and sizes its launches before any device call (the boxes /
 * boxes_host precedent of par_stft_pan_ratio_f32).  Column ranges lie in [0, n_frames], lo <= hi, and each is either equal to its
 * predecessor's or starts at or behind its predecessor's end; row ranges lie in [0, bins], in any order, and may overlap, their
 * lengths summing to at most bins + height.  width, height in [1, PAR_IMAGE_MAX_SIDE].
 * peak (DEVICE f32) is column-major like the frame-major spectrogram: cell (c, r) at peak[c * pitch + r], pitch >= height; nothing
 * but those cells (r < height) and scratch is written.
 *
 * par_stft_peak_image_f32 (fused): peak[c][r] = the maximum over frames f in [cols[c]) and bins b in [rows[r]) of the float32
 * magnitude m_f[b] par_stft_f32 mode 1 writes for the channel view x[i * x_stride] (DEVICE f32, n samples; `window` DEVICE
 * f32[n_fft]) -- padding, framing, the repeated reflection of a signal shorter than n_fft/2, scaling and the + 1e-7f included --
 * with bins = n_fft*zeropad/2 + 1 and n_frames = par_stft_frames(n, n_fft, hop).  A cell with no frame or no bin is 0.0f.  No
 * spectrogram is stored; only frames some column names are transformed, and a column equal to its predecessor is transformed
 * once.  The maximum is taken on the magnitudes' bit patterns as unsigned integers (they are positive floats; every NaN is first
 * made 0x7fc00000, above all of them): a NaN magnitude makes its cell NaN, as np.max does, and the result is equal bit for bit to
 * par_peak_image_f32 on the stored spectrogram, from run to run and whatever the launch shape.  Long columns are cut into chunks of
 * at most R = max(16, ceil(F / 16384)) frames, F the frames the distinct columns name (a column of L frames into ceil(L / R)
 * nearly equal parts): a rule of the arguments alone.  The call zero-fills the image, a column of one chunk is stored, and the
 * chunks of a longer column meet through a vector atomic unsigned maximum on the zero-filled cells (no partial rows, no reduce
 * kernel; a maximum has no order).  scratch: DEVICE, 8-byte aligned, par_stft_peak_image_scratch_bytes(width) = one int64 per
 * column and one more, needs no initialisation.  n_fft*zeropad must be a power of two in [16, 16384] and n_fft even, otherwise
 * PAR_ERR_UNSUPPORTED (compose par_stft_big_f32 mode 1 and par_peak_image_f32).  Null pointers; n, hop, zeropad, x_stride, width or
 * height < 1; a side above PAR_IMAGE_MAX_SIDE; pitch < height; misaligned scratch; a table that breaks the rules above:
 * PAR_ERR_ARG.  scratch_bytes too small: PAR_ERR_WORKSPACE.  All before any device call. */
#define PAR_IMAGE_MAX_SIDE (1 << 19)
/* Bytes of DEVICE scratch (host arithmetic; 0 for a width outside [1, PAR_IMAGE_MAX_SIDE]) */
size_t par_stft_peak_image_scratch_bytes(int64_t width);
int par_stft_peak_image_f32(int device, const float* x, int64_t n, int64_t x_stride, int n_fft, int hop, int zeropad,
                            const float* window, const int64_t* cols, const int64_t* cols_host, const int32_t* rows,
                            const int32_t* rows_host, int64_t width, int64_t height, float* peak, int64_t pitch, void* scratch,
                            size_t scratch_bytes, void* stream);
/* par_peak_image_f32 (composed): the same cells from a STORED frame-major float32 magnitude spectrogram, a chunk at a time: mag
 * (DEVICE f32 [n_frames_chunk][mag_pitch], mag_pitch >= bins) holds frames frame_first .. frame_first + n_frames_chunk of the
 * n_frames the tables speak of (what par_stft_f32 and par_stft_big_f32 write in mode 1).  Every cell is MAXIMISED with the chunk's
 * part of it, peak[c][r] = max(peak[c][r], max over the column's frames inside the chunk and the row's bins), on the same bit
 * patterns as above: the caller zero-fills the image before the first chunk, chunks may arrive in any order and their seams may
 * fall inside a column.  One thread owns a cell per launch: no atomics.  n_frames_chunk == 0: PAR_OK, nothing done.  Null
 * pointers, bins < 1, mag_pitch < bins, a chunk outside [0, n_frames], sides outside [1, PAR_IMAGE_MAX_SIDE], pitch < height, a
 * table that breaks the rules: PAR_ERR_ARG before any device call. */
int par_peak_image_f32(int device, const float* mag, int64_t mag_pitch, int64_t bins, int64_t n_frames, int64_t frame_first,
                       int64_t n_frames_chunk, const int64_t* cols, const int64_t* cols_host, const int32_t* rows,
                       const int32_t* rows_host, int64_t width, int64_t height, float* peak, int64_t pitch, void* stream);
/* par_image_colorize_u8: out (DEVICE u8, ROW-major [height][width][4], row 0 first; 4-byte aligned) = lut[idx] (lut DEVICE
 * u8[256][4], 4-byte aligned, passed through byte for byte) with, in float64,
 *   dB = 20 log10((double) m)   m = peak[c * pitch + r], the logarithm of par_band_mean_db_f32
 *   t = (dB - vmin) / (vmax - vmin);  idx = (int) floor(min(max(t, 0), 1) * 255 + 0.5)
 * m == 0 (no data) or NaN gives (0, 0, 0, 0).  Against numpy's log10 an index can differ by one only where t * 255 + 0.5 lies within
 * 1e-12 of an integer.  Null pointers, sides outside [1, PAR_IMAGE_MAX_SIDE], pitch < height, vmin >= vmax or not finite,
 * misaligned lut or out: PAR_ERR_ARG before any device call. */
int par_image_colorize_u8(int device, const float* peak, int64_t width, int64_t height, int64_t pitch, double vmin, double vmax,
                          const uint8_t* lut, uint8_t* out, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* PAR_HIP_H */
