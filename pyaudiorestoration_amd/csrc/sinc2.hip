// K_sinc, streaming form -- the north-star kernel: NT = 32 files, mono on unit strides (k_sinc_pipe<1, 2> + <1, 1>: two kernels by
// stream kind, r06), the two channels of an interleaved stereo file (k_sinc_pipe<2, 0>, r05), one channel of such a file (<2, 3>,
// r06); k_sinc_pipe_n<...>: the same bodies over the streams of up to eight files in one launch (r06).
//
// Semantics: resampling.sinc_core (reference util/resampling.py:51-90), fused with the speed curve like k_sinc_fused (sinc.hip).
//
// Shape.  ONE WAVE = one worker that streams over 9-23 (an odd number of) consecutive 1024-output tiles of the file; waves never meet (no
// workgroup, no barrier).  A pass takes the next 128 outputs (two per lane), places them from the plan's block records, and
// evaluates their windows against ONE 128-centre stretch of the input grid [ws, ws + 128), ws = the first centre rounded down
// to 8; outputs whose centre lies beyond it (a handful: periods differ from 1 by <= 1.25 %) simply open the next pass.
//   * taps 3 <= |n| <= 31 at fc = 1: a Farrow bank in q = shift^2 (minimax polynomials of (win_n/pi)/(n^2 - q),
//     tools/sinc2_model.py) -- six fixed FIR filters on the input grid, evaluated for the pass's 128 centres on the matrix cores
//     (v_mfma_f32_16x16x32_f16, signal and dominant filter pair split float16 hi + lo 2^-12: 13 MFMAs since r06, 11 since r11 --
//     the third K slice, 8 % full, folded into one product: see bank_load); the bank goes through the wave's own LDS and every
//     output gathers its centre's row;
//   * fc < 1 (read head slower than the output clock) = the fc = 1 result + a correction in g = 1 - fc whose taps are ENTIRE
//     functions of g (n - s): all 63 taps enter through seven fixed MOMENT filters m_i = sum_n (-1)^n win_n (n/32)^i x[c + n]
//     on the same image (18 more MFMAs to order 6, with the bank's 13 unfolded: 31; 13 more to order 5 where every lane of the pass
//     has g <= 0.0105, the (m0 m1) pair's third slice folded like the bank's: 24, r11) and a complex Horner in 32 pi g per output (tools/sinc3_model.py; 1e-7 of the peak for
//     g <= 0.0101, 5e-7 to 0.0125; steeper tiles go to the block kernel).  One image, per-lane g exact, no restarts;
//   * the constant fragments of both filter sets RESIDENT IN REGISTERS for the life of the wave: 21 + the two folded ones (the fc = 1
//     kernel <1, 1>: 8 + 1); a pass of the order-6 loop swaps the folded ones for the four slice-2 fragments it still multiplies by;
//   * taps |n| <= 2 on the vector units with the lane's exact shift (two reciprocals per output);
//   * the input streams through a ring per wave (8 chunks of 128 float32 samples, direct-to-LDS loads two passes ahead),
//     converted ONCE to float16 hi / lo images for the banks -- no halo is ever re-read or re-converted; block records of the
//     passes ahead are fetched while the current one computes.
// What the record model or float16 do not cover goes to the block kernel through a tile list (k_sinc_fused_list / _list2,
// sinc.hip): blocks flagged slow, outputs within the reference's own rounding of a half-integer position (window-centre ties),
// input that is non-finite / >= 32 / all but silent.  The file's END tiles (the ring would reach over the file's ends) are
// not streamed at all: the launch's first workgroups do them the block kernel's way (fused_wave, sinc_block.h) beside the
// streams.  Every window centre is the reference's rint(p) either way.
// Stereo (k_sinc_pipe<2>): the ring holds frames (left, right); a pass is placed ONCE and both channels are converted, banked
// and gathered for it -- in ONE set of bank rows, which the channels take turns in (the order of the loop's stages and the
// one-chunk lag of channel 1's image: see the loop) so that eight streams still fit a compute unit's LDS; outputs leave as
// 8-byte frames.  177 -> 133 vector instructions per channel-sample.
// History: r04 built this kernel in four forms (a pass as a chain of stages; the pipelined loop with the fc < 1 taps as two
// MODULATED images of the signal; an fc = 1-only kernel at three waves per SIMD; the moment form, also as workgroups of several
// streams sharing the constants through LDS).  NOTES r04 has their numbers; the product carries the one that won.
#define PAR_WANT_BANK2 1
#include "par_common.h"
#include "pos_plan.h"
#include "sinc_taps_gen.h"
#include "sinc_common.h"
#define PAR_COLD_FN __forceinline__      // (the end tiles' float64 cold functions inline: no private segment for the streaming kernels)
#include "sinc_block.h"           // fused_wave: the file's end tiles are done the block kernel's way by the launch's first workgroups
#ifndef PAR_COLD_FN_GIVEN
#error "sinc_block.h was included before PAR_COLD_FN was defined: the cold functions would stay out of line"
#endif
#include <algorithm>
#include <atomic>
#include <limits.h>
#include <type_traits>

constexpr int kMaxTilesPerWave = 23;          // k_sinc_pipe's tiles per wave for long files (launch_sinc_stream picks 8 .. this)
#ifndef PAR_S2_EXP
#define PAR_S2_EXP 0            // timing builds, never shipped: 1 no MFMAs, 2 no near taps, 4 no stores, 8 no conversion, 16 unity maths on every pass
#endif

namespace par {

typedef _Float16 half8v __attribute__((ext_vector_type(8)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float float4v __attribute__((ext_vector_type(4)));

constexpr int kRing = 512;                       // samples per ring (float32 and float16 images alike)
constexpr int kPass = 128;                       // centres per pass = outputs tried per pass
// The float16 images hold the signal x kImgScale (r06).  A sample's hi part is zero -- and the sample then reaches only the
// filters that take the lo image -- below 6e-8 instead of 6e-5, i.e. practically never: passages 60 dB down lose nothing (their
// zero crossings used to), and the (e1 d1) filters no longer need the lo image at all (2 MFMAs per pass; without the scale a
// signal at 1e-3 came out 4.5e-5 wrong, tools/sinc2_model.py).  The price is the streaming kernel's range: |x| < 32 (beyond it the
// lo part of the scaled sample leaves float16; such tiles are the block kernel's).
constexpr float kImgScale = 1024.0f, kImgScaleInv = 0.0009765625f;
constexpr float kImgMax = 32.0f;                 // |x| the images can hold
// A chunk whose loudest sample is below 2^-13 (and not 0) is the block kernel's, as before the scale: a sample with a zero hi part
// (below 6e-8) loses its (e1 d1) and m2.. contributions, ~2e-3 of what it adds to an output -- 1.2e-10, which must stay below
// 1e-6 of the passage's own level (a file at 1e-6 came out 1.9e-4 wrong with the threshold scaled down, test_unity_path_matrix_core_bank)
constexpr float kQuiet = 0.0001220703125f;


#if PAR_S2_EXP & 64
__device__ unsigned long long* g_s2_phase;       // [waves][16] cycle sums per phase (timing builds only)
#define S2_MARK(k)                                              \
  do {                                                          \
    const unsigned long long now_ = __builtin_readcyclecounter(); \
    ph_[k] += now_ - pt_;                                       \
    pt_ = now_;                                                 \
  } while (0)
#else
#define S2_MARK(k) do { } while (0)
#endif

struct S2Args {
  int64_t len_out;
  const float* sig;
  int64_t len_in;
  float* out;
  const TileHdr* hdr;
  const BlockRec* rec;
  const BlockRec2* rec2;
  int* redo_count;
  int* redo_list;
  int tiles;                                     // tiles per wave (k_sinc_pipe; <= 48: a lane per tile header)
  int tiles_tail;                                // ... of the streams behind the first n_big (the launch's last round: short
  int64_t n_big;                                 // streams, so that the GPU does not idle behind a few long ones)
  int64_t n_full;                                // full tiles of the file
  int64_t n_tiles;                               // tiles with a header
  // The file's END tiles -- the first (its ring would reach in front of the file), the last two full ones (... behind it) and the
  // partial one -- are not streamed: the launch's first n_edge workgroups do them the block kernel's way (fused_wave, sinc_block.h),
  // 128 outputs each, BESIDE the streams.  (Through the tile list they cost 50 us behind every launch: cold code -- the masked
  // path of the last wave, the float64 slow path of the first outputs -- fetched by one wave while the GPU idles, r05.)
  int n_edge;
  int64_t out_stride;                            // k_sinc_pipe<2, 3> only (one channel of frames): elements between two outputs
  FusedArgs fa;
  const float4* tab;
  TapModes tmd;
};
constexpr int kEdgeWaveOut = 128;                                   // outputs per end-tile workgroup (one wave)
constexpr int kEdgeWavesPerTile = kSincTileOutputs / kEdgeWaveOut;
constexpr int kTileEdge = 0x100;                                    // (kernel-local header flag: an end tile, nobody pushes it)

__device__ __forceinline__ float sinpi_poly(float z) {       // sin(pi x) / x as a polynomial in z = x^2, |x| <= 0.52
  float p = -0.00737043094f;
  p = fmaf(p, z, 0.0821458866f);
  p = fmaf(p, z, -0.599264529f);
  p = fmaf(p, z, 2.55016404f);
  p = fmaf(p, z, -5.16771278f);
  return fmaf(p, z, 3.14159265f);
}

// hi part of the float16 split.  The matrix cores flush subnormal float16 operands to zero (measured: a modulated image lost
// its samples below 6.1e-5 near the modulator's zero crossings, 2e-5 of the peak): below float16's normal range the hi part is
// zero and the lo part (x 4096) carries the value.  (Switching the wave to flush float16 subnormals, MODE.FP_DENORM[3:2] = 0,
// would make the conversions do this for free -- tools/exp/denorm_mode.hip -- but the bank's packed e2 / d2 halves of a quiet
// passage ARE subnormal and must survive: 7.7e-5 of the block's peak on the 'loud next to quiet' test with the mode set.)
__device__ __forceinline__ _Float16 hi16(float x) { return (_Float16)(fabsf(x) < 6.103515625e-05f ? 0.0f : x); }
#define S2_HI(x) hi16(x)

__device__ __forceinline__ unsigned pack_h2(float a, float b) {
  const half2v h = {(_Float16)a, (_Float16)b};
  return __builtin_bit_cast(unsigned, h);
}
__device__ __forceinline__ float h_lo(unsigned w) { return (float)__builtin_bit_cast(half2v, w)[0]; }
__device__ __forceinline__ float h_hi(unsigned w) { return (float)__builtin_bit_cast(half2v, w)[1]; }


// Direct-to-LDS loads as inline assembly: LDS address = M0 + 4 (or 16) x lane.  Through the compiler's builtin every later LDS
// read that might alias the destination gets an s_waitcnt vmcnt(0) in front of it -- the very latency the stream is built to
// hide.  Issued this way the compiler does not count them; the kernel waits for them itself (one vmcnt(0) at the head of a
// pass, when they are a whole pass old).
// The destination is a 32-bit LDS ADDRESS (lds_addr() of the stream's LDS, once per wave, plus a member's offset): handed over
// as a generic pointer every call paid the cast's null check in front of its s_mov m0 (r09).
__device__ __forceinline__ unsigned lds_addr(const void* lds) {
  return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) void*)lds;
}
__device__ __forceinline__ void dma_dword(const float* gptr, const unsigned la) {
  asm volatile("s_mov_b32 m0, %1\n\tglobal_load_lds_dword %0, off" ::"v"(gptr), "s"(__builtin_amdgcn_readfirstlane(la)) : "memory", "m0");
}
__device__ __forceinline__ void dma_dwordx4(const void* gptr, const unsigned la) {
  asm volatile("s_mov_b32 m0, %1\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(gptr), "s"(__builtin_amdgcn_readfirstlane(la)) : "memory", "m0");
}

// 128 consecutive floats from a wave-uniform address (b, as an integer): two direct loads off a scalar base (per-lane byte offset 4 l; the instruction
// offset advances the global and the LDS address alike)
__device__ __forceinline__ void dma_chunk128(const unsigned long long b, unsigned lane_bytes, const unsigned la) {
  const unsigned long long bs = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(b >> 32)) << 32) |
                                (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b);       // (the value IS wave-uniform)
  asm volatile("s_mov_b32 m0, %2\n\tglobal_load_lds_dword %0, %1\n\tglobal_load_lds_dword %0, %1 offset:256"
               ::"v"(lane_bytes), "s"(bs), "s"(__builtin_amdgcn_readfirstlane(la)) : "memory", "m0");
}

// 128 stereo frames (256 consecutive floats): four direct loads
__device__ __forceinline__ void dma_chunk256(const unsigned long long b, unsigned lane_bytes, const unsigned la) {
  const unsigned long long bs = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(b >> 32)) << 32) |
                                (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b);
  asm volatile("s_mov_b32 m0, %2\n\tglobal_load_lds_dword %0, %1\n\tglobal_load_lds_dword %0, %1 offset:256\n\t"
               "global_load_lds_dword %0, %1 offset:512\n\tglobal_load_lds_dword %0, %1 offset:768"
               ::"v"(lane_bytes), "s"(bs), "s"(__builtin_amdgcn_readfirstlane(la)) : "memory", "m0");
}

__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Lane sets of a pass are PREFIXES of its 128 outputs (indices and window centres increase with the lane): they live as
// counts in scalar registers, a lane tests one with a single compare, and the set algebra is SALU work.
__device__ __forceinline__ int clamp64(int n) { return n < 0 ? 0 : (n > 64 ? 64 : n); }
__device__ __forceinline__ unsigned long long prefix(int n) { return n >= 64 ? ~0ull : ((1ull << n) - 1ull); }   // 0 <= n <= 64

// Placement of one row (64 consecutive outputs, lane l) from its block records (pos_plan.h BlockRec): window centre relative
// to A0, sub-sample shift, max(period - 1, 0); bad() = the lane's block leaves the plain record model (a slow piece, the cubic
// term: flags of its record word m) or its centre lies within the reference's own rounding of a tie -- such tiles go to the block
// kernel.  The word and the tie test leave separately: the loop ORs the two rows' words and tests the flags once (r10).
constexpr unsigned kRecBadFlags = kRecSlow0 | kRecSlow1 | kRecCubic;
struct S2Row {
  int c;
  float s, ep;
  unsigned m;
  bool tie;
  __device__ __forceinline__ bool bad() const { return (m & kRecBadFlags) != 0u || tie; }
};
template <bool SECOND = true>                    // false: the caller knows that no lane of the row takes its block's second piece
__device__ __forceinline__ S2Row s2_place_row(const uint4 ra, const uint4 rb, const int u, const int cbase, const float uf,
                                              const float u2f, const float tw1, const float tw0, const float tolf) {
  const unsigned m = ra.x;
  const bool second = SECOND && (unsigned)u > (m & 31u);
  const float F = __uint_as_float(second ? rb.y : ra.y), e1 = __uint_as_float(second ? rb.z : ra.z),
              e2 = __uint_as_float(second ? rb.w : ra.w);
  const int irel = (int)(second ? rb.x : ra.x) >> 16;
  const bool last = (unsigned)u == ((m >> kRecLastShift) & 63u);
  const float frac = fmaf(u2f, e2, fmaf(uf, e1, F));
  const float e = fmaf(e2, last ? tw0 : tw1, e1);               // period to the next position, minus 1
  const float ri = rintf(frac);
  S2Row o;
  o.s = frac - ri;
  o.c = cbase + irel + (int)ri;
  o.ep = __builtin_amdgcn_fmed3f(e, 0.0f, 3.0e38f);             // max(e, 0) in one instruction
  o.m = m;
  o.tie = !(fabsf(fabsf(o.s) - 0.5f) > tolf);                   // (two compares per pass: a float minimum of the rows would drop a NaN)
  return o;
}


// ------------------------------------------------------------------------------------------------------------------------
// The loop.  Run as a chain -- records -> placement -> conversion -> bank -> gather, a wait for LDS or memory between every two
// links -- a pass took 4 360 cycles for ~350 instructions at the two waves per SIMD the registers allow (r04, first shape).
// Here the links of one iteration belong to DIFFERENT passes:
//     iteration k:   OUT(k)        gather + near taps + stores of the pass placed and banked in iteration k - 1
//                    PLACE(k + 1)  from records that set out in iteration k - 2
//                    BANK(k + 1)   over the centres PLACE(k + 1) just named, from image chunks converted in iterations <= k - 1
//                    CONV          the next 128-sample chunk of the ring (fetched in iteration k - 2) -> float16 images
//                    FETCH         chunk + 2 of the ring and the records of pass k + 3 set out (direct-to-LDS loads)
// so nothing an iteration reads from LDS was written in the same iteration: ONE wave-level fence per iteration, one
// s_waitcnt vmcnt(5) (everything but the previous iteration's five memory operations has landed), no branch in the body.
// The ring holds 8 chunks of float32 samples (near taps) and 4 of the float16 images; the bank is single-buffered (an
// iteration's gathers precede its bank writes in program order, LDS serves a wave's operations in order).
// Order of one iteration of the MONO loop at two waves per SIMD (k_sinc_pipe<1, 2>, r08; the fc = 1 kernel <1, 1> at four waves, the
// one-channel kernel <2, 3> and the stereo loop keep the order above).  At four waves a wave that waits for its own LDS read is
// covered by the other three; at two it is not, so every read is issued a stage ahead of its use:
//     wait vmcnt + fence
//     READS    the records of PLACE(k + 1), CONV's ring chunk, the gathers of OUT(k) (3 rows + 5 ring samples per output):
//              their addresses are loop state, the data landed before the fence
//     PLACE(k + 1) behind a partial lgkmcnt (the records alone); the loop's exit margin -- scalar instructions only, every
//              minimum pinned to a scalar register (r10) -- rides beside it.  Seven passes in eight lie inside one tile and
//              take both rows' anchor from one add; the pass that straddles a tile border selects per lane in a block of
//              its own, behind a scalar branch and out of the loop's line
//     READS    BANK(k + 1)'s image fragments (fc = 1: five, xv among them; fc < 1: six), as soon as ws is known
//     OUT(k)   arithmetic, pinned here: the fragments land under it -- both rows in the fc = 1 and the order-6 loop; in the
//              order-5 loop (the benchmark's fc < 1 passes) the first row only
//     BANK(k + 1) MFMAs -- order 5: OUT(k)'s second row dealt out behind them, two vector instructions to an MFMA (which hides
//              that many) -- then the row writes (behind OUT(k)'s gathers); CONV arithmetic + image writes (behind the
//              fragment reads)
//     FETCH, DMA, stores (one 32-bit byte offset per pass off the stream's scalar base, row 1 as the instruction offset), fence
// Same hazards as above -- nothing read that the iteration wrote, gathers before row writes, fragment reads before image writes,
// one fence, one vmcnt wait -- and the same arithmetic expressions: the outputs are bit-identical to the r06 order's (NOTES r08).
// (tools/isa_census.py --waits lists each read, the wait that covers it and the wave's own vector work in between.)
// Whatever is not the plain case -- the first pass of a run, a pass that meets a flagged tile or block, the end of the
// wave's range, a change of tap regime, a conversion window that has drifted out of its slack -- leaves the loop
// and is done by start_run(): the same stages, one after the other with full waits, which also primes the loop again.
constexpr int kRingF = 1024;                      // float32 samples in the ring (8 chunks)
constexpr int kRingH = 512;                       // samples per float16 image (4 chunks)

// A stream's LDS.  NCH = 2: an interleaved stereo file -- the ring holds frames (left, right), each channel has its own float16
// images, and the two channels take turns in ONE set of bank rows (see the loop of k_sinc_pipe).
// MOM = false: the stream of a kernel that only knows fc = 1 passes (k_sinc_pipe<1, 1>) -- no moment rows, the packed e2 | d2
// halves in an array of their own: 9.8 KB, sixteen streams per compute unit.
template <int NCH, bool MOM = true>
struct S3Lds {
  static constexpr bool kMoments = MOM;
  float ring_head[4 * NCH];                      // frames -2, -1 mirror frames 1022, 1023
  float ring[kRingF * NCH];
  float ring_tail[4 * NCH];                      // mirrors frames 0 .. 3
  _Float16 img[2 * NCH][kRingH];                 // x hi, lo x 4096 (stereo: [2 ch], [2 ch + 1])
  float4v qa[kPass];                             // bank rows {e0, d0, e1, d1}, slot = ci ^ ((ci >> 3) & 7)
  float4v qm0[MOM ? kPass : kPass / 4];          // moment rows {m0, m1, m2, e2|d2 (halves)} (same slots); !MOM: e2|d2 alone, a float per slot
  float4v qm1[MOM ? kPass : 1];                  // {m3, m4, m5, m6}
  __device__ __forceinline__ float& e2d2(int sl) {
    return MOM ? reinterpret_cast<float*>(&qm0[sl])[3] : reinterpret_cast<float*>(&qm0[0])[sl];
  }
  __device__ __forceinline__ const float& e2d2(int sl) const {
    return MOM ? reinterpret_cast<const float*>(&qm0[sl])[3] : reinterpret_cast<const float*>(&qm0[0])[sl];
  }
#ifdef PAR_S3_LDS_PAD
  uint4 pad[PAR_S3_LDS_PAD / 16];                // (occupancy experiments)
#endif
  uint4 recs[4][16];                             // block records of four passes: [0..7] first pieces, [8..15] second pieces
};
static_assert(offsetof(S3Lds<1>, img) % 16 == 0 && offsetof(S3Lds<1>, qa) % 16 == 0 && offsetof(S3Lds<1>, recs) % 16 == 0, "16-byte aligned");
static_assert(offsetof(S3Lds<2>, ring) % 16 == 0 && offsetof(S3Lds<2>, img) % 16 == 0 && offsetof(S3Lds<2>, qa) % 16 == 0 &&
              offsetof(S3Lds<2>, recs) % 16 == 0, "16-byte aligned");
static_assert(sizeof(S3Lds<2>) <= 20480, "eight stereo streams per compute unit (160 KB of LDS)");
using S3LdsUnity = S3Lds<1, false>;
static_assert(sizeof(S3LdsUnity) <= 10240 && offsetof(S3LdsUnity, recs) % 16 == 0 && offsetof(S3LdsUnity, qa) % 16 == 0,
              "sixteen fc = 1 streams per compute unit");

struct S3Pass {                                  // a placed pass: 128 candidate outputs j .. j + 127 (two per lane)
  int cw[2];                                     // window centre relative to ws: the row's bank slot before its clamp to 0 .. 127 (r10: what
                                                 // the placement's nok test works out and OUT uses; the centre itself has no other reader)
  float s[2], ep[2];                             // shift, max(period - 1, 0)
  int nok[2];                                    // lanes of row r the pass finishes: l < nok[r]   (wave-uniform)
  int j, ws;                                     // first output (relative to Ja), first bank centre (wave-uniform)
};

// fc = 1 bank AND the seven moment filters of the fc < 1 correction over the same 128 centres, from the same signal fragments:
// 13 + 18 MFMAs to order 6, 11 + 13 to order 5, 11 for the bank alone.  fr: the fc = 1 bank's ten constant fragments (kBank2Frags32's
// first ten), fmr: the moment filters' fifteen (kBank3Frags32, sinc_taps_gen.h), both without the dominant pairs' slice 2, which
// is fsw's (below); resident in the wave's registers.  MOMENTS = false: the fc = 1 bank alone.
constexpr int kCtabUnity = 10;
// SIX = false: without the moment of order 6 (passes with 1 - fc <= 0.0105: the series to order 5 is within 1.6e-6 there)
// (in two halves: the signal fragments read from the images -- five, six with the moment filters -- and the matrix work with the row writes)
struct S3Frags {
  half8v xh[3], xl[3];
  half8v xv;                                     // the folded slice 2's mixed fragment (below)
};
// The third K slice folded (r11).  Slice 2 of a filter pair holds only the overhang -- taps 33 - i .. 31 of sub-position i >= 2: K
// entries 64 .. 69, lanes g = 0 of its fragments, 42 of 512 elements; lanes 16-63 are zero (tools/sinc2_model.py asserts it) --
// and a K index only has to mean the same thing in A and B.  So the dominant pair's three slice-2 products (hi hi; lo hi and
// hi lo) are ONE MFMA into the lo accumulator: the constant fragment V (kBank2FoldFrag32 / kBank3FoldFrag32) carries under K
// group g = 0 the pair's hi slice 2 x 4096 (exact in float16; the accumulator's 2^-12 brings it back), g = 1 its lo slice 2,
// g = 2 its hi slice 2, g = 3 zeros; the signal fragment xv has image samples 64 .. 71 of the lane's block under every group --
// the lo image's in the lanes g = 2, the hi image's elsewhere (xv_img: the lane's block and image as byte offsets, formed once
// per run of a loop; the images are a power of two long, so the image is OR-ed behind the ring's mask: two vector instructions
// for the address).
// FOLD passes read neither xl[2] nor, without the moment filters, xh[2].  The order-6 loop keeps its three full slices.
struct S3XvLane {
  unsigned at, img;                              // bytes: the lane's block + K entry 64 in an image; the lane's image
};
__device__ __forceinline__ S3XvLane bank_xv_img(const int l) {
  return S3XvLane{16u * (unsigned)(l & 15) + 64u * (unsigned)sizeof(_Float16), (l >> 4) == 2 ? (unsigned)(kRingH * sizeof(_Float16)) : 0u};
}
template <bool FOLD, bool XH2, class LDS>
__device__ __forceinline__ S3Frags bank_load(const LDS& L, const int offs, const int l, const S3XvLane xv_img, const int ch = 0) {
  const int bb = l & 15, g = l >> 4;
  // (byte offsets into an image, masked as bytes: as element indices every fragment's address paid a shift behind its mask)
  constexpr unsigned kImgBytes = kRingH * sizeof(_Float16);
  const unsigned b0 = (unsigned)offs * (unsigned)sizeof(_Float16) + 16u * (unsigned)(bb + g);
  const char* const hi = reinterpret_cast<const char*>(&L.img[2 * ch][0]);
  const char* const lo = reinterpret_cast<const char*>(&L.img[2 * ch + 1][0]);
  S3Frags X;
#pragma unroll
  for (int ks = 0; ks < 3; ++ks) {
    const unsigned at = (b0 + 64u * ks) & (kImgBytes - 1u);
    X.xh[ks] = X.xl[ks] = half8v{};
    if (ks < 2 || !FOLD || XH2) X.xh[ks] = *reinterpret_cast<const half8v*>(hi + at);
    if (ks < 2 || !FOLD) X.xl[ks] = *reinterpret_cast<const half8v*>(lo + at);
  }
  X.xv = half8v{};
  if constexpr (FOLD) {
    static_assert(sizeof(L.img[0]) == kImgBytes, "the lo image lies kImgBytes behind the hi image");
    const unsigned at = (((unsigned)offs * (unsigned)sizeof(_Float16) + xv_img.at) & (kImgBytes - 1u)) | xv_img.img;
    X.xv = *reinterpret_cast<const half8v*>(hi + at);
  }
  return X;
}
// fsw: the four constant fragments that depend on the loop -- folded passes: {V2, V3, -, -}; order 6: slice 2 of (e0 d0) hi, lo and
// of (m0 m1) hi, lo (fragments 2, 7 of the bank, 2, 5 of the moment filters), which fr / fmr do not hold
constexpr bool bank_folds(bool moments, bool six) { return !(moments && six); }
template <bool MOMENTS, bool SIX = true, class LDS>
__device__ __forceinline__ void bank_math(LDS& L, const half8v (&fr)[kBank2Frags], const half8v (&fmr)[kBank3Frags],
                                          const half8v (&fsw)[4], const S3Frags& X, const int l) {
  constexpr bool FOLD = bank_folds(MOMENTS, SIX);
  constexpr int NS = FOLD ? 2 : 3;               // full slices of the dominant pairs
  const int bb = l & 15, g = l >> 4;
  const half8v (&xh)[3] = X.xh, (&xl)[3] = X.xl;
  auto frag = [&](int f) {
    return f == 2 ? fsw[0] : f == 7 ? fsw[1] : f == kCtabUnity + 2 ? fsw[2] : f == kCtabUnity + 5 ? fsw[3] : f < kCtabUnity ? fr[f] : fmr[f - kCtabUnity];
  };
  const float4v z = {0.0f, 0.0f, 0.0f, 0.0f};
  float4v e0 = z, lo = z, e1 = z, e2 = z;
#pragma unroll
  for (int ks = 0; ks < NS; ++ks) {
    const half8v f0 = frag(ks);
    e0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(f0, xh[ks], e0, 0, 0, 0);
    lo = __builtin_amdgcn_mfma_f32_16x16x32_f16(frag(5 + ks), xh[ks], lo, 0, 0, 0);
    lo = __builtin_amdgcn_mfma_f32_16x16x32_f16(f0, xl[ks], lo, 0, 0, 0);
    if (ks < 2) {
      const half8v f1 = frag(3 + ks);
      e1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(f1, xh[ks], e1, 0, 0, 0);      // (no lo image here since the images are scaled, r06)
      e2 = __builtin_amdgcn_mfma_f32_16x16x32_f16(frag(8 + ks), xh[ks], e2, 0, 0, 0);
    }
  }
  if constexpr (FOLD) lo = __builtin_amdgcn_mfma_f32_16x16x32_f16(fsw[0], X.xv, lo, 0, 0, 0);      // slice 2: hi hi x 4096 + lo hi + hi lo
  // (the factor in a vector register: a VALU instruction with an SGPR operand issues at 4.3 cycles instead of 2.4, tools/exp/valu_forms.hip)
  float lo_inv = kBank2LoInv;
  asm volatile("" : "+v"(lo_inv));
  const float4v v0 = e0 + lo * lo_inv, v1 = e1;
  float4v a01 = z, l01 = z, a23 = z, a45 = z, a6 = z;
  if (MOMENTS) {
    if constexpr (FOLD) l01 = __builtin_amdgcn_mfma_f32_16x16x32_f16(fsw[1], X.xv, l01, 0, 0, 0);
#pragma unroll
    for (int ks = 0; ks < 3; ++ks) {
      if (ks < NS) {
        const half8v f01 = frag(kCtabUnity + ks);
        a01 = __builtin_amdgcn_mfma_f32_16x16x32_f16(f01, xh[ks], a01, 0, 0, 0);
        l01 = __builtin_amdgcn_mfma_f32_16x16x32_f16(frag(kCtabUnity + 3 + ks), xh[ks], l01, 0, 0, 0);
        l01 = __builtin_amdgcn_mfma_f32_16x16x32_f16(f01, xl[ks], l01, 0, 0, 0);
      }
      a23 = __builtin_amdgcn_mfma_f32_16x16x32_f16(frag(kCtabUnity + 6 + ks), xh[ks], a23, 0, 0, 0);
      a45 = __builtin_amdgcn_mfma_f32_16x16x32_f16(frag(kCtabUnity + 9 + ks), xh[ks], a45, 0, 0, 0);
      if constexpr (SIX) a6 = __builtin_amdgcn_mfma_f32_16x16x32_f16(frag(kCtabUnity + 12 + ks), xh[ks], a6, 0, 0, 0);
    }
  }
  const float4v m01 = a01 + l01 * lo_inv;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int sl = (8 * bb + 2 * g + p) ^ (bb & 7);
    const float4v row = {v0[2 * p], v0[2 * p + 1], v1[2 * p], v1[2 * p + 1]};
    L.qa[sl] = row;
    const float e2d2 = __uint_as_float(pack_h2(e2[2 * p] * 0.015625f, e2[2 * p + 1] * 0.015625f));
    if constexpr (MOMENTS) {
      const float4v r0 = {m01[2 * p], m01[2 * p + 1], a23[2 * p], e2d2};
      L.qm0[sl] = r0;
      const float4v r1 = {a23[2 * p + 1], a45[2 * p], a45[2 * p + 1], a6[2 * p]};
      L.qm1[sl] = r1;
    } else {
      L.e2d2(sl) = e2d2;
    }
  }
}
template <bool MOMENTS, bool SIX = true, class LDS>
__device__ __forceinline__ void bank_image3m(LDS& L, const half8v (&fr)[kBank2Frags], const half8v (&fmr)[kBank3Frags],
                                             const half8v (&fsw)[4], const int offs, const int l, const S3XvLane xv_img, const int ch = 0) {
  bank_math<MOMENTS, SIX>(L, fr, fmr, fsw, bank_load<bank_folds(MOMENTS, SIX), MOMENTS>(L, offs, l, xv_img, ch), l);
}

// the outputs of one row of a placed pass (bank and ring in LDS): MODE 1 fc = 1, MODE 3 fc = 1 + the
// moment correction  -g (cos(pi s) Re Q - sin(pi s) Im Q),  Q = sum_i M_i (i 32 G)^i (alpha_i + i beta_i),  G = pi g, w = G s,
// alpha_i = 1/(i! (i+1)) - w^2 / (2 i! (i+3)),  beta_i = -w / (i! (i+2))   (tools/sinc3_model.py: 1e-7 for g <= 0.0101)
// (in two halves: the LDS reads of a row -- its bank and moment rows, the five ring samples of the near taps -- and the
// arithmetic on them; the mono loop issues the reads at the head of an iteration and works them out a stage later)
struct S3Gather {
  float4v row, M0, Mh;                           // {e0, d0, e1, d1}, {m0, m1, m2, e2|d2}, {m3 .. m6}  (MODE 1: M0[3] alone)
  float xm2, xm1, x0, xp1, xp2;
};
template <int MODE, int NCH = 1, class LDS>
__device__ __forceinline__ S3Gather s3_out_load(const LDS& L, const int ci, const int wsK, const int ch = 0) {
  const int sl = ci ^ ((ci >> 3) & 7);
  const int rc = (wsK + ci) & (kRingF - 1);
  const float* xp = &L.ring[NCH * rc + ch];
  S3Gather G;
  G.xm2 = xp[-2 * NCH], G.xm1 = xp[-NCH], G.x0 = xp[0], G.xp1 = xp[NCH], G.xp2 = xp[2 * NCH];
  G.row = L.qa[sl];
  G.M0 = float4v{0.0f, 0.0f, 0.0f, 0.0f};
  G.Mh = G.M0;
  if constexpr (MODE != 1) {
    G.M0 = L.qm0[sl];
    G.Mh = L.qm1[sl];
  } else {
    G.M0[3] = L.e2d2(sl);
  }
  return G;
}
template <int MODE>
__device__ __forceinline__ float s3_out_math(const S3Gather& Gr, const float sr, const float epr) {
  using T32 = TapTab<32>;
  constexpr float kUs = kBank2ScaleInv * kImgScaleInv;      // bank rows -> signal units
  constexpr float kMs = kImgScaleInv;                       // moment rows -> signal units (rides in the Horner's constants)
  const float xm2 = Gr.xm2, xm1 = Gr.xm1, x0 = Gr.x0, xp1 = Gr.xp1, xp2 = Gr.xp2;
  const float q = sr * sr, q64 = 64.0f * q;
  const float R1 = fast_rcp(fmaf(q, T32::B[1], T32::A[1])), R2 = fast_rcp(fmaf(q, T32::B[2], T32::A[2]));
  {
    const float E1 = xp1 + xm1, D1 = xp1 - xm1, E2 = xp2 + xm2, D2 = xp2 - xm2;
    const float4v row = Gr.row;
    const float4v M0 = Gr.M0;
    const unsigned w2 = __float_as_uint(M0[3]);
    const float e = fmaf(q, fmaf(q64, h_lo(w2), row[2]), row[0]), d = fmaf(q, fmaf(q64, h_hi(w2), row[3]), row[1]);
    const float en = fmaf(E2, R2, -(E1 * R1));
    const float dn = fmaf(D2 + D2, R2, -(D1 * R1));
    const float et = fmaf(e, kUs, en), dt = fmaf(d, kUs, dn);
    const float spq = sinpi_poly(q);                                  // sin(pi s) / s
    const float unity = spq * fmaf(-sr, fmaf(sr, et, dt), x0 * 0.318309886f);
    if constexpr (MODE == 1) return unity;
    else {
    const float4v Mh = Gr.Mh;
    const float m3 = Mh[0], m4 = Mh[1], m5 = Mh[2], m6 = Mh[3];
    const float g = epr * fast_rcp(1.0f + epr);                        // 1 - fc
    const float G = 3.14159265f * g, w = G * sr, w2m = w * w, G32 = 32.0f * G;
    float re, im;
    if constexpr (MODE == 3) {
      // i = 6 (beta_6 and the w^2 terms of i >= 3 are below 1e-8 of the peak)
      re = m6 * (1.98412698e-4f * kMs);                                // 1 / (6! 7)
      im = 0.0f;
    } else {                                                           // MODE 2: the series to order 5 (1 - fc <= 0.0105)
      re = m5 * (1.38888889e-3f * kMs);                                // i = 5: 1/(5! 6), 1/(5! 7)
      im = m5 * (w * -(1.19047619e-3f * kMs));
    }
#define S3_MOM_STEP(Mi, A0, A1, B0)                                   \
    {                                                                 \
      const float al_ = (A1) != 0.0f ? fmaf(w2m, -((A1) * kMs), (A0) * kMs) : (A0) * kMs, be_ = w * -((B0) * kMs);      /* (A1 = 0: no fma with -0.0) */ \
      const float nre_ = fmaf(-G32, im, (Mi) * al_), nim_ = fmaf(G32, re, (Mi) * be_); \
      re = nre_;                                                      \
      im = nim_;                                                      \
    }
    if constexpr (MODE == 3) S3_MOM_STEP(m5, 1.38888889e-3f, 0.0f, 1.19047619e-3f)             // i = 5: 1/(5! 6), -, 1/(5! 7)
    S3_MOM_STEP(m4, 8.33333333e-3f, 0.0f, 6.94444444e-3f)             // i = 4: 1/(4! 5), -, 1/(4! 6)
    S3_MOM_STEP(m3, 4.16666667e-2f, 0.0f, 3.33333333e-2f)             // i = 3: 1/(3! 4), -, 1/(3! 5)
    S3_MOM_STEP(M0[2], 1.66666667e-1f, 5.0e-2f, 1.25e-1f)             // i = 2: 1/(2! 3), 1/(2 2! 5), 1/(2! 4)
    S3_MOM_STEP(M0[1], 0.5f, 0.125f, 3.33333333e-1f)                  // i = 1: 1/2, 1/(2 4), 1/3
    S3_MOM_STEP(M0[0], 1.0f, 1.66666667e-1f, 0.5f)                    // i = 0: 1, 1/(2 3), 1/2
#undef S3_MOM_STEP
    const float S = sr * spq, C = __builtin_amdgcn_cosf(0.5f * sr);
    return fmaf(-g, fmaf(C, re, -(S * im)), unity);
    }
  }
}
template <int MODE, int NCH = 1, class LDS>
__device__ __forceinline__ float s3_out_row(const LDS& L, const int ci, const float sr, const float epr, const int wsK, const int ch = 0) {
  return s3_out_math<MODE>(s3_out_load<MODE, NCH>(L, ci, wsK, ch), sr, epr);
}

// one chunk of the ring -> float16 images (and the ring's mirrors); returns false when float16 does not suit the chunk
// (in two halves like a row's gather: the lane's two ring samples, and the arithmetic with the image writes)
// A chunk is named by its first window index w0 = 128 x chunk (what the loop carries, r09).  The verdict is a lane MASK, zero
// when float16 suits the chunk: bitwise on the three ballots, so that no branch is compiled for it and a caller can OR it
// into its other masks.
// The ring's mirrors -- frames 0 .. 3 behind frame 1023, frames 1022, 1023 in front of frame 0: each behind a scalar branch on
// the chunk's slot with the lane test inside (six chunks in eight pass both by; as two exec-masked blocks they ran their mask
// algebra in every iteration).
__device__ __forceinline__ unsigned long long s3_convert_verdict(const float x0, const float x1) {
  const float am = fmaxf(fabsf(x0), fabsf(x1));
  // (each ballot straight from ONE compare, the masks combined on the scalar unit: a ballot of `a || b` went through a bool in a
  // vector register -- v_cndmask 0, 1 and a compare with 0 again -- in k_sinc_pipe<1, 1>, r10)
  const unsigned long long big = __builtin_amdgcn_ballot_w64(!(fabsf(x0) < kImgMax)) | __builtin_amdgcn_ballot_w64(!(fabsf(x1) < kImgMax));       // (also set for NaN)
  const unsigned long long loud = __builtin_amdgcn_ballot_w64(am >= kQuiet), some = __builtin_amdgcn_ballot_w64(am > 0.0f);
  return big | (loud == 0ull ? some : 0ull);
}
template <int NCH, class LDS, class V>
__device__ __forceinline__ void s3_ring_mirrors(LDS& L, const int w0, const int l, const int ix, const V xx) {
  const int slot = w0 & (7 * kPass);                        // (wave-uniform)
  // (the wave barrier -- no instruction -- keeps the compiler from folding the slot test into the lane mask again)
  if (slot == 0) {
    __builtin_amdgcn_wave_barrier();
    if (l < 2) *reinterpret_cast<V*>(&L.ring_tail[NCH * ix]) = xx;
  }
  if (slot == 7 * kPass) {
    __builtin_amdgcn_wave_barrier();
    if (l == kWave - 1) *reinterpret_cast<V*>(&L.ring_head[2 * NCH]) = xx;
  }
}
template <class LDS>
__device__ __forceinline__ float2 s3_convert_load(const LDS& L, const int w0, const int l) {
  const int ix = (w0 + 2 * l) & (kRingF - 1);
  return *reinterpret_cast<const float2*>(&L.ring[ix]);
}
template <class LDS>
__device__ __forceinline__ unsigned long long s3_convert_math(LDS& L, const int w0, const int l, const float2 xx) {
  const int wi = w0 + 2 * l;
  const int ix = wi & (kRingF - 1), ih = wi & (kRingH - 1);
  const float x0 = xx.x, x1 = xx.y;
  const unsigned long long trouble = s3_convert_verdict(x0, x1);
  s3_ring_mirrors<1>(L, w0, l, ix, xx);
  const float s0 = x0 * kImgScale, s1 = x1 * kImgScale;
  const half2v h = {S2_HI(s0), S2_HI(s1)};
  const half2v lo = {(_Float16)((s0 - (float)h[0]) * 4096.0f), (_Float16)((s1 - (float)h[1]) * 4096.0f)};
  *reinterpret_cast<half2v*>(&L.img[0][ih]) = h;
  *reinterpret_cast<half2v*>(&L.img[1][ih]) = lo;
  return trouble;
}
template <class LDS>
__device__ __forceinline__ unsigned long long s3_convert(LDS& L, const int w0, const int l) {
  return s3_convert_math(L, w0, l, s3_convert_load(L, w0, l));
}

// Stereo ring (frames left, right): channel `ch` of one chunk -> that channel's float16 images.  `mirrors`: the call also keeps the
// ring's mirror frames (both channels': the caller converts channel 0 of a chunk first).
template <class LDS>
__device__ __forceinline__ unsigned long long s3_convert_ch(LDS& L, const int w0, const int l, const int ch, const bool mirrors) {
  const int wi = w0 + 2 * l;
  const int ix = wi & (kRingF - 1), ih = wi & (kRingH - 1);
  const float4v xx = *reinterpret_cast<const float4v*>(&L.ring[2 * ix]);
  const float x0 = ch ? xx[1] : xx[0], x1 = ch ? xx[3] : xx[2];
  const unsigned long long trouble = s3_convert_verdict(x0, x1);
  if (mirrors) s3_ring_mirrors<2>(L, w0, l, ix, xx);
  const float s0 = x0 * kImgScale, s1 = x1 * kImgScale;
  const half2v h = {S2_HI(s0), S2_HI(s1)};
  const half2v lo = {(_Float16)((s0 - (float)h[0]) * 4096.0f), (_Float16)((s1 - (float)h[1]) * 4096.0f)};
  *reinterpret_cast<half2v*>(&L.img[2 * ch][ih]) = h;
  *reinterpret_cast<half2v*>(&L.img[2 * ch + 1][ih]) = lo;
  return trouble;
}

// fc < 1 passes are fc = 1 + the moment correction (one image per channel, per-lane 1 - fc exact): valid for 1 - fc <= 0.0125,
// steeper tiles go to the block kernel's list.  (r04's other forms -- a pass as a chain of stages, the modulated-image form of
// the fc < 1 taps, an fc = 1-only kernel at three waves per SIMD, workgroups of several streams sharing the constants through
// LDS -- are in the repository's history and in NOTES r04 with their numbers; the product carries this one.)
constexpr float kEpMaxMom = 0.0125f / (1.0f - 0.0125f);      // period - 1 at 1 - fc = 0.0125
// Passes whose lanes all have 1 - fc <= 0.0105 take the moment series to order 5 (regime 2: no m6 -- three matrix-core
// instructions and a Horner step per pass; within 1.6e-6 of the peak on a Nyquist tone there, 5.5e-6 at 0.0125: tools/sinc3_model.py);
// the order-6 loop (regime 3) keeps a stream until its passes fall below 0.95 of that (no flapping between the loops)
constexpr float kEpMom5 = 0.0105f / (1.0f - 0.0105f), kEpMom5Lo = 0.95f * kEpMom5;
#ifndef PAR_S3_SHARE_OUT
#define PAR_S3_SHARE_OUT 1      // stereo: 0 = channel 1's row arithmetic worked out afresh (measured: 158 against 165 G on the benchmark's tape)
#endif
#ifndef PAR_S3_PIN_MONO
#define PAR_S3_PIN_MONO 0       // 1: the mono loop's row results pinned like the stereo loop's (234 instead of 250 registers, 1 % slower)
#endif
// KIND: which streams of the launch the kernel takes, and what it has to know for them (r06).  A wave issues an instruction
// every ~5 cycles whatever its kind, so two waves per SIMD -- what the 25 constant fragments of both filter sets leave room
// for -- cannot fill the SIMD's issue slots; a stream whose tiles hold fc = 1 outputs only needs the fc = 1 bank's ten:
//   0  every stream, both tap regimes (stereo: its LDS allows two streams per SIMD either way)
//   1  the streams WITHOUT a tile the plan marks kTileMaySlow: fc = 1 passes only, 10 fragments, no moment rows in LDS:
//      three waves per SIMD.  (A pass with an fc < 1 lane after all -- the hint is conservative, this does not happen -- sends
//      its tile to the block kernel's list.)
//   2  the streams with such a tile: both regimes, as KIND 0
//   3  (NCH = 2) ONE channel of an interleaved two-channel file -- the reference's use_channels, a strided column view
//      (util/resampling.py:211-227): the ring holds the frames as they lie in memory (a.sig = the wanted channel's first sample:
//      it is channel 0 of the frames that start there), conversion, bank and gather take that channel only, the loop is the
//      mono one; outputs a.out_stride elements apart.  Every stream, both regimes.
// A mono file is launched as KIND 2 and KIND 1 back to back over the same grid; a wave of the wrong kind leaves at once.
// (the body of the kernel: workgroup `bx` of one file's launch -- k_sinc_pipe has one file, k_sinc_pipe_n up to eight)
template <int NCH, int KIND>
__device__ __forceinline__ void sinc_pipe_body(const S2Args& a, const int bx, S3Lds<NCH, KIND != 1>& L) {
  static_assert(NCH == 1 || NCH == 2, "mono, or an interleaved stereo file");
  static_assert(KIND == 0 || KIND == 3 || NCH == 1, "the stereo form takes every stream");
  static_assert(KIND != 3 || NCH == 2, "one channel of FRAMES");
  constexpr bool kPick = KIND == 3;               // one channel of two-channel frames: stereo ring, mono loop
  constexpr bool kTwo = NCH == 2 && !kPick;       // both channels of a pass: the stereo loop
  constexpr bool kMom = KIND != 1;
  // the mono loop at two waves per SIMD: its LDS reads a stage ahead (see the loop)
  constexpr bool kEarly = NCH == 1 && KIND == 2;
  const int l = threadIdx.x & (kWave - 1);
  if (bx < a.n_edge) {                            // an end tile's wave: tile 0, then n_full - 2, n_full - 1 and the partial one
    if constexpr (KIND == 1) return;              // (done by the launch of the other kind)
    else {
    const int e = bx / kEdgeWavesPerTile, w = bx % kEdgeWavesPerTile;
    const int64_t T = e == 0 ? 0 : a.n_full - 3 + e;
    const int64_t jw = T * kSincTileOutputs + (int64_t)w * kEdgeWaveOut;
    const int nrem = (int)(a.len_out - jw < (int64_t)kEdgeWaveOut ? (a.len_out - jw > 0 ? a.len_out - jw : 0) : kEdgeWaveOut);
    float* const piece = reinterpret_cast<float*>(&L);
    static_assert(sizeof(L) >= fused_capw(2 * NCH, NCH) * NCH * sizeof(float), "the wave's span fits the stream's LDS");
    if constexpr (kPick) {                        // a strided view: the block kernel's general path, 128 outputs per wave too
      static_assert(sizeof(L) >= fused_capw(2, 1) * sizeof(float), "the wave's span fits the stream's LDS");
      if (nrem > 0)
        fused_wave<1, 32, 2, false>(a.len_out, a.sig, nullptr, 2, a.len_in, 32, a.tab, a.tmd, a.out, nullptr, a.out_stride, a.fa, piece, l,
                                    jw, nrem, piece);
      return;
    }
    if (nrem == kEdgeWaveOut)
      fused_wave<NCH, 32, 2 * NCH, true>(a.len_out, a.sig, a.sig + 1, NCH, a.len_in, 32, a.tab, a.tmd, a.out, a.out + 1, NCH, a.fa, piece, l,
                                         jw, nrem, piece);
    else if (nrem > 0)
      fused_wave<NCH, 32, 2 * NCH, false>(a.len_out, a.sig, a.sig + 1, NCH, a.len_in, 32, a.tab, a.tmd, a.out, a.out + 1, NCH, a.fa, piece, l,
                                          jw, nrem, piece);
    return;
    }
  }
  const int64_t stream_id = (int64_t)bx - a.n_edge;
  const int my_tiles = stream_id < a.n_big ? a.tiles : a.tiles_tail;
  const int64_t Ta = stream_id < a.n_big ? stream_id * a.tiles : a.n_big * a.tiles + (stream_id - a.n_big) * a.tiles_tail;
  if (Ta >= a.n_full) return;
  const int64_t Tb = Ta + my_tiles < a.n_full ? Ta + my_tiles : a.n_full;
  const int64_t Ja = Ta * kSincTileOutputs, Jb = Tb * kSincTileOutputs;
  long long A0;
  int hd_dA, hd_fl;
  {
    const int64_t Ti = Ta + l < a.n_tiles ? Ta + l : a.n_tiles - 1;
    const TileHdr h = a.hdr[l <= my_tiles ? Ti : Ta];
    // (lane 0's anchor through readfirstlane, not a shuffle: the compiler takes a shuffle's result for lane-variant, and with A0
    // everything derived from it -- the ring's source, the chunks inside the file, dma_bad, hence the loop's exit test and every
    // piece of state the loop carries -- sat in vector registers behind exec-masked branches, r06)
    A0 = (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned long long)h.anchor >> 32)) << 32) |
                     (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long long)h.anchor));
    const long long d = h.anchor - A0;
    hd_fl = h.flags | ((d > -0x40000000ll && d < 0x40000000ll) ? 0 : 1);
    if (a.n_edge > 0 && (Ta + l == 0 || Ta + l >= a.n_full - 2)) hd_fl |= 1 | kTileEdge;      // end tiles: not streamed, not pushed
    hd_dA = (int)d;
    if constexpr (KIND == 1 || KIND == 2) {       // is this stream the kernel's kind?
      const bool any_slow = __ballot(l < my_tiles && Ta + l < Tb && (h.flags & kTileMaySlow) != 0) != 0ull;
      if (any_slow != (KIND == 2)) return;
    }
  }
  // the fc = 1 bank's constant fragments and the moment filters' (kinds 0 and 2), but for the four slice-2 fragments of the
  // dominant pairs: those are fsw's, which holds what the current loop needs of them (bank_math)
  half8v fr[kBank2Frags];
  {
    const uint4* src = reinterpret_cast<const uint4*>(kBank2Frags32) + l;
#pragma unroll
    for (int f = 0; f < kBank2Frags; ++f) fr[f] = f == 2 || f == 7 ? half8v{} : __builtin_bit_cast(half8v, src[f * kWave]);
  }
  half8v fmr[kBank3Frags];
  if constexpr (kMom) {
    const uint4* src = reinterpret_cast<const uint4*>(kBank3Frags32) + l;
#pragma unroll
    for (int f = 0; f < kBank3Frags; ++f) fmr[f] = f == 2 || f == 5 ? half8v{} : __builtin_bit_cast(half8v, src[f * kWave]);
  }
  // fsw holds {V2, V3} but for a pass of regime 3, around which it is loaded with the four slice-2 fragments and with the folded ones
  // again: a stream meets the order-6 loop rarely (never in the benchmark's files), and all 27 fragments resident would not leave
  // the loops the registers they are scheduled in at two waves per SIMD.
  half8v fsw[4] = {half8v{}, half8v{}, half8v{}, half8v{}};
  auto fsw_load = [&](bool six) {
    // (the lane as a value of this call's own: loads of constants at an address the loops do not change are hoisted out of
    // them, and all six fragments stay resident after all)
    int ll = l;
    asm volatile("" : "+v"(ll));
    const uint4* const b2 = reinterpret_cast<const uint4*>(kBank2Frags32) + ll;
    const uint4* const b3 = reinterpret_cast<const uint4*>(kBank3Frags32) + ll;
    if (six) {
      fsw[0] = __builtin_bit_cast(half8v, b2[2 * kWave]);
      fsw[1] = __builtin_bit_cast(half8v, b2[7 * kWave]);
      fsw[2] = __builtin_bit_cast(half8v, b3[2 * kWave]);
      fsw[3] = __builtin_bit_cast(half8v, b3[5 * kWave]);
    } else {
      fsw[0] = __builtin_bit_cast(half8v, reinterpret_cast<const uint4*>(kBank2FoldFrag32)[ll]);
      if constexpr (kMom) fsw[1] = __builtin_bit_cast(half8v, reinterpret_cast<const uint4*>(kBank3FoldFrag32)[ll]);
    }
  };
  fsw_load(false);
  {
    uint4* z = reinterpret_cast<uint4*>(&L.img[0][0]);
    const uint4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < (int)(sizeof(L.img) / 16 / kWave); ++i) z[i * kWave + l] = zero;
  }
  const float tolf = (float)((fabs((double)A0) + 2.0e7) * 1.2e-16 + 2.0e-10) + 2.0e-7f;
  const int nJ = (int)(Jb - Ja);
  float* const outW = a.out + (kPick ? a.out_stride : (int64_t)NCH) * Ja;
  const uint4* const recW = reinterpret_cast<const uint4*>(a.rec) + (Ja >> kRecShift);
  const uint4* const rec2W = reinterpret_cast<const uint4*>(a.rec2) + (Ja >> kRecShift);
  const int blk_max = (int)(((a.len_out + kRec - 1) >> kRecShift) - (Ja >> kRecShift)) - 1;      // last block with a record, relative

  // ---- stream state (wave-uniform) ----
  int j0 = 0;                                    // first output not yet placed into a finished pass
  // dma_bad: the first chunk of the ring that does not lie inside the file (set where the ring is restarted: chunks are issued
  // in increasing order from 0, so it is known from the file's ends); capped well above any chunk a ring reaches (a ring is
  // restarted 2^20 samples behind its base) so that 128 x dma_bad stays an int
  constexpr int kDmaBadMax = 1 << 22;
  int wbase = 0, conv_next = 0, conv_lo = 0, dma_next = 0, dma_bad = 0, mode = 0, pk = 0;
  int regime = 1;                                // the loop the current pass belongs to: 1 fc = 1, 2 / 3 fc = 1 + the moment correction to order 5 / 6
                                                 // (mode: 1 = the float16 images in LDS follow the ring, 0 = to be rebuilt)
  int rbA = 0, rbB = 0, rbC = 0;                 // first block (relative) of the record buffers of passes pk + 1, pk + 2, pk + 3

  // records: lanes 0-7 fetch first pieces, 8-15 second pieces, one 16-byte direct load each.  (The plan's record arrays end four
  // tiles behind the file's last block -- fused_blocks(), pos_plan.h -- so the 16 blocks a guess may reach past it are readable.)
  const uint4* const rec_lane = (l < 8 ? recW : rec2W) + (l & 7);
  using LdsT = S3Lds<NCH, KIND != 1>;
  const unsigned lds_base = lds_addr(&L);        // direct loads name their LDS destination by address: one cast per wave
  const unsigned lds_recs = lds_base + (unsigned)offsetof(LdsT, recs), lds_ring = lds_base + (unsigned)offsetof(LdsT, ring);
  constexpr unsigned kRecBufBytes = 16 * sizeof(uint4);              // one pass's records in LDS
  constexpr unsigned kChunkBytes = kPass * NCH * sizeof(float);      // one chunk of the ring, in LDS as in memory
  // (rbytes: the buffer as its byte offset in L.recs, kRecBufBytes x (pass & 3) -- what the loop carries)
  auto fetch_records_at = [&](unsigned rbytes, int blk0) {           // 8 first pieces + 8 second pieces from block blk0 on
    if (l < 16) dma_dwordx4(rec_lane + (blk0 < 0 ? 0 : blk0), lds_recs + rbytes);
  };
  auto fetch_records = [&](int buf, int blk0) { fetch_records_at(kRecBufBytes * (unsigned)buf, blk0); };
  // ring chunks: chunk k = input samples [wbase + 128 k, + 128) relative to A0 -> ring slot k & 7.  Chunks 0 .. dma_bad - 1 lie
  // inside the file; the others are never used and fetch some readable stretch instead.
  unsigned long long ring_src = (unsigned long long)(uintptr_t)a.sig;      // &sig[A0 + wbase], as an integer
  auto ring_restart = [&]() {
    const long long o = A0 + wbase;
    ring_src = (unsigned long long)(uintptr_t)a.sig + (unsigned long long)((long long)(NCH * sizeof(float)) * o);
    // (one channel of frames: the last frame's second word may lie one float behind the caller's view -- never fetched)
    const long long khi = ((long long)a.len_in - (kPick ? 1 : 0) - o) / kPass - 1;      // last chunk that ends inside the file
    dma_bad = o < 0 || khi < 0 ? 0 : (int)(khi + 1 > kDmaBadMax ? kDmaBadMax : khi + 1);
  };
  const unsigned lane_bytes = 4u * (unsigned)l;
  // (src: &chunk; the fallback a.sig is readable: len_in >= 128 for every file this kernel is launched on)
  auto chunk_dma_at = [&](bool inside, unsigned long long src, unsigned slot_bytes) {
    const unsigned long long s = inside ? src : (unsigned long long)(uintptr_t)a.sig;
    if constexpr (NCH == 2) dma_chunk256(s, lane_bytes, lds_ring + slot_bytes);
    else dma_chunk128(s, lane_bytes, lds_ring + slot_bytes);
  };
  auto chunk_dma = [&](int k) {                  // the cold path's form; the loop carries the source and the slot
    chunk_dma_at(k < dma_bad, ring_src + (unsigned long long)((long long)kChunkBytes * k), (unsigned)(k & 7) * kChunkBytes);
  };
  auto push_tile = [&](int64_t T) {
    if (l == 0) {
      const int slot = atomicAdd(a.redo_count, 1);
      a.redo_list[slot] = (int)T;
    }
  };
  if (stream_id == 0 && a.n_full < a.n_tiles && a.n_edge == 0) push_tile(a.n_full);

  // placement of the pass that starts at output j from record buffer `buf` (first block rb); the lanes' tile anchors
  struct Placed {
    S2Row R[2];
    int nt[2];
    int fl0, fl1, tend;
    int epm;                                     // the larger period - 1 of the lane's two outputs, as its bit pattern (ep >= 0: ordered like the floats)
  };
  // anchors and flags of the tile of j and of the one behind it, refreshed once per tile.  j only ever grows over a wave's life,
  // so "another tile" is j >= tc_tend (the cached tile's end; 0: nothing cached); tc_flm: the loop's exit margin of the two
  // flags, negative for a flagged tile
  int tc_tend = 0, tc_dA0 = 0, tc_dA1 = 0, tc_fl0 = 0, tc_fl1 = 0, tc_flm = 0;
  struct PlaceRecs {
    uint4 ra0, rb0, ra1, rb1;                    // first / second pieces of the blocks of the lane's two outputs
    int t5;                                      // (j & 31) + l, which named them: the placement takes it from here
  };
  // (rbytes: the record buffer as its byte offset in L.recs; jb = (j >> kRecShift) - rb, the pass's first block in the buffer --
  // the loop's exit test needs it too, so the loop works it out once)
  auto place_load = [&](int j, unsigned rbytes, int jb) {
    const int t5 = (j & (kRec - 1)) + l;
    const int bi = (jb + (t5 >> kRecShift)) & 7;
    const uint4* rp = &L.recs[0][0] + (rbytes >> 4);
    return PlaceRecs{rp[bi], rp[8 + bi], rp[(bi + 2) & 7], rp[8 + ((bi + 2) & 7)], t5};
  };
  // (EARLY: the records were read ahead by place_load; otherwise they are read here, where the compiler keeps the second pieces'
  // reads inside the variant that selects them)
  auto place_impl = [&](int j, unsigned rbytes, int jb, auto early, const PlaceRecs& RR) {
    Placed P;
    if (j >= tc_tend) {
      const int T = j >> 10;
      tc_tend = (T + 1) << 10;
      tc_dA0 = __builtin_amdgcn_readlane(hd_dA, T);
      tc_dA1 = __builtin_amdgcn_readlane(hd_dA, T + 1);
      tc_fl0 = __builtin_amdgcn_readlane(hd_fl, T);
      tc_fl1 = __builtin_amdgcn_readlane(hd_fl, T + 1);
      tc_flm = -((tc_fl0 | tc_fl1) & 1);
    }
    P.tend = tc_tend;
    const int dA0 = tc_dA0, dA1 = tc_dA1;
    P.fl0 = tc_fl0;
    P.fl1 = tc_fl1;
    uint4 ra0, rb0, ra1, rb1;
    int t5;
    if constexpr (decltype(early)::value) {
      ra0 = RR.ra0, rb0 = RR.rb0, ra1 = RR.ra1, rb1 = RR.rb1, t5 = RR.t5;
    } else {
      t5 = (j & (kRec - 1)) + l;
      const int bi = (jb + (t5 >> kRecShift)) & 7;
      const uint4* rp = &L.recs[0][0] + (rbytes >> 4);
      ra0 = rp[bi], rb0 = rp[8 + bi], ra1 = rp[(bi + 2) & 7], rb1 = rp[8 + ((bi + 2) & 7)];
    }
    const int u = t5 & (kRec - 1);
    const int uc = u - kRec / 2;
    const float uf = (float)uc, u2f = uf * uf, tw1 = fmaf(2.0f, uf, 1.0f), tw0 = tw1 - 2.0f;
    // lanes of the two rows that lie in the tile of j: l < nt[r] (a lane's compare needs no clamp; the cold path's masks clamp)
    P.nt[0] = P.tend - j;
    P.nt[1] = P.tend - j - 64;
    // The rows' tile anchors.  Seven passes in eight lie inside the tile of j (a scalar test): both rows count from its anchor.
    // The pass that straddles a tile border selects per lane, behind a scalar BRANCH (the wave barrier -- no instruction -- keeps
    // the compiler from folding the test into the lanes' selects again, as in s3_ring_mirrors): as a select alone every pass
    // paid two copies of the anchors into vector registers, a compare and a select per row (r10).
    int cb0 = dA0 + uc, cb1 = cb0;
    if (__builtin_expect(P.nt[0] < kPass, 0)) {
      __builtin_amdgcn_wave_barrier();
      cb0 = (l < P.nt[0] ? dA0 : dA1) + uc;
      cb1 = (l < P.nt[1] ? dA0 : dA1) + uc;
    }
    // a segment starts inside one block in eight: most passes have no second piece to select
    if (__ballot((unsigned)u > (ra0.x & 31u) || (unsigned)u > (ra1.x & 31u)) == 0ull) {
      P.R[0] = s2_place_row<false>(ra0, rb0, u, cb0, uf, u2f, tw1, tw0, tolf);
      P.R[1] = s2_place_row<false>(ra1, rb1, u, cb1, uf, u2f, tw1, tw0, tolf);
    } else {
      P.R[0] = s2_place_row(ra0, rb0, u, cb0, uf, u2f, tw1, tw0, tolf);
      P.R[1] = s2_place_row(ra1, rb1, u, cb1, uf, u2f, tw1, tw0, tolf);
    }
    // (one integer maximum serves the regime test and the moment correction's limit: two compares where there were a float
    // maximum with its quieting moves and three; ep is fmed3(e, 0, 3e38): never NaN, -0 sorts below everything)
    P.epm = max(__float_as_int(P.R[0].ep), __float_as_int(P.R[1].ep));
    return P;
  };
  auto place = [&](int j, int buf, int rb) {
    return place_impl(j, kRecBufBytes * (unsigned)buf, (j >> kRecShift) - rb, std::false_type{}, PlaceRecs{});
  };

  S3Pass P;                                      // the pass OUT works on next (placed, its bank in LDS)
  P.nok[0] = P.nok[1] = 0;
  P.j = P.ws = 0;
  P.cw[0] = P.cw[1] = 0;
  P.s[0] = P.s[1] = P.ep[0] = P.ep[1] = 0.0f;

  auto out_pass = [&](auto mode_tag, const S3Pass& Q, float (&res)[2], const int ch = 0) {
    constexpr int MODE = decltype(mode_tag)::value;
    const int wsK = Q.ws - wbase;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      int ci = Q.cw[r];
      ci = ci < 0 ? 0 : (ci > kPass - 1 ? kPass - 1 : ci);
      float sr = Q.s[r], epr = Q.ep[r];
#if !PAR_S3_SHARE_OUT
      // (experiment: channel 1's row arithmetic hidden from the common-subexpression pass.  By default the compiler keeps the
      // channel-independent values of a row -- reciprocals, sin(pi s)/s, the moment step's coefficients -- from channel 0's turn)
      if (NCH == 2 && ch == 1) asm volatile("" : "+v"(sr), "+v"(epr));
#endif
      res[r] = s3_out_row<MODE, NCH>(L, ci, sr, epr, wsK, ch);
    }
  };
  // The unit-stride stores: ONE 32-bit byte offset per pass, (j + l) elements, off the stream's scalar base outW; row 1 is the
  // instruction offset 64 elements further on.  (Indexed as outW[j + 64 r + l] every row's address was widened to 64 bits in
  // vector registers, r10.)  The strided one-channel form keeps its 64-bit index.
  static_assert(48ull * kSincTileOutputs * sizeof(float2) + 2 * kWave * sizeof(float2) < (1ull << 32),
                "the largest stream (48 tiles of stereo frames) stays below 2^32 bytes");
  auto out_bytes = [&](auto elem, int j) -> size_t { return (size_t)(((unsigned)j + (unsigned)l) * (unsigned)sizeof(elem)); };
  auto store_pass = [&](const S3Pass& Q, const float (&res)[2]) {
#pragma unroll
    for (int r = 0; r < 2; ++r)
      if (l < Q.nok[r] && !(PAR_S2_EXP & 4)) {
        if constexpr (kPick) outW[(int64_t)((unsigned)Q.j + 64u * r + (unsigned)l) * a.out_stride] = res[r];
        else *reinterpret_cast<float*>(reinterpret_cast<char*>(outW) + out_bytes(float{}, Q.j) + kWave * sizeof(float) * r) = res[r];
      }
  };
  auto store_pass2 = [&](const S3Pass& Q, const float (&res0)[2], const float (&res1)[2]) {      // stereo: a frame per lane and row
#pragma unroll
    for (int r = 0; r < 2; ++r)
      if (l < Q.nok[r] && !(PAR_S2_EXP & 4))
        *reinterpret_cast<float2*>(reinterpret_cast<char*>(outW) + out_bytes(float2{}, Q.j) + kWave * sizeof(float2) * r) = make_float2(res0[r], res1[r]);
  };
  // one chunk of the ring -> float16 image(s); stereo: both channels of the chunk
  // (w0 = 128 x chunk; returns the lane mask of s3_convert_verdict: zero when the chunk suits float16)
  auto convert_chunk = [&](int w0) -> unsigned long long {
    if constexpr (kPick) {
      return s3_convert_ch(L, w0, l, 0, true);
    } else if constexpr (NCH == 2) {
      const unsigned long long t0 = s3_convert_ch(L, w0, l, 0, true);
      const unsigned long long t1 = s3_convert_ch(L, w0, l, 1, false);
      return t0 | t1;
    } else {
      return s3_convert(L, w0, l);
    }
  };

  // ---- the cold path: places, converts for, banks and -- unless it is a full pass the loop can take -- finishes the pass
  // at j0, everything in order with full waits.  Returns the regime of P = a full pass ready for the loop (records of the two
  // passes behind it and the ring's next two chunks landed), 0 when the range is done.
#if PAR_S2_EXP & 128
#define S3_COUNT(k) do { if (l == 0) atomicAdd(a.redo_count + (k), 1); } while (0)
#else
#define S3_COUNT(k) do { } while (0)
#endif
  auto start_run = [&]() -> int {
    for (;;) {
      if (j0 >= nJ) return 0;
      S3_COUNT(1);
      __builtin_amdgcn_s_waitcnt(0x0F70);
      wave_lds_fence();
      const int buf = pk & 3;
      fetch_records(buf, j0 >> kRecShift);
      __builtin_amdgcn_s_waitcnt(0x0F70);
      wave_lds_fence();
      const Placed Q = place(j0, buf, j0 >> kRecShift);
      const int tend = Q.tend;
      // lane sets: valid lanes (inside the range), lanes of this tile
      int nv[2] = {clamp64(nJ - j0), clamp64(nJ - j0 - 64)};
      // the moment correction covers 1 - fc <= 0.0125
      const unsigned long long b0 = __ballot(Q.R[0].bad() || !(Q.R[0].ep <= kEpMaxMom)) & prefix(nv[0]),
                               b1 = __ballot(Q.R[1].bad() || !(Q.R[1].ep <= kEpMaxMom)) & prefix(nv[1]);
      const int nt0 = clamp64(Q.nt[0]), nt1 = clamp64(Q.nt[1]);
      const unsigned long long bad_here = (b0 & prefix(nt0)) | (b1 & prefix(nt1));
      const bool bad_next = ((b0 & ~prefix(nt0)) | (b1 & ~prefix(nt1)) | (unsigned long long)((Q.fl1 & 1) && tend < nJ)) != 0ull;
      if (bad_next) {                             // the pass ends at the tile border
        nv[0] = nv[0] < nt0 ? nv[0] : nt0;
        nv[1] = nv[1] < nt1 ? nv[1] : nt1;
      }
      bool skip = (Q.fl0 & 1) || bad_here != 0ull;
      const unsigned long long gen = (__ballot(1.0f + Q.R[0].ep != 1.0f) & prefix(nv[0])) | (__ballot(1.0f + Q.R[1].ep != 1.0f) & prefix(nv[1]));
      const int ws = __builtin_amdgcn_readfirstlane(Q.R[0].c) & ~7;
      S3Pass N;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        N.cw[r] = Q.R[r].c - ws;
        N.s[r] = Q.R[r].s;
        N.ep[r] = Q.R[r].ep;
        const unsigned long long in = __ballot(N.cw[r] < kPass);
        N.nok[r] = __popcll(in & prefix(nv[r]));
      }
      N.j = j0;
      N.ws = ws;
      const unsigned long long steep = (__ballot(Q.R[0].ep > kEpMom5) & prefix(nv[0])) | (__ballot(Q.R[1].ep > kEpMom5) & prefix(nv[1]));
      const int want = gen == 0ull ? 1 : (steep == 0ull ? 2 : 3);      // the pass's regime
      if (!kMom && want != 1) skip = true;        // (a kernel of fc = 1 streams met an fc < 1 lane: the block kernel's tile)
      if (!skip) {
        bool rebuild = mode != 1;
        // the ring: restarted at the first pass of the wave and after a jump the fetched chunks do not cover
        const int lo_need = ws - 39 - wbase;      // window index of the first image sample the bank reads
        if (mode == 0 || lo_need < kPass * (dma_next - 8) + kPass || lo_need < 0 || lo_need > kPass * dma_next || ws - wbase > (1 << 20)) {
          __builtin_amdgcn_s_waitcnt(0x0F70);     // (nothing may still be on its way into the old ring)
          wbase = ws - 39;
          dma_next = 0;
          rebuild = true;
          ring_restart();                         // (names dma_bad for the new ring)
        }
        const int wsK = ws - wbase;
        regime = want;
        if (rebuild) {
          mode = 1;
          conv_lo = conv_next = (wsK - 39) >> 7;
        }
        // slack of the conversion window.  The loop checks the pass BEHIND this one (its bank needs the image to reach
        // 161 samples beyond its first centre, one pass = 120 .. 136 centres further on) and converts one chunk per
        // iteration: fc = 1 passes advance by <= 128 centres (the converted stretch drifts ahead of them: start low),
        // fc < 1 passes by >= 128 (start as far ahead as the four-chunk image ring allows)
        const int conv_target = want == 1 ? (wsK + 300 + 127) >> 7 : (wsK + 465) >> 7;
        const int need_lo = (wsK - 39) >> 7;      // first image chunk the bank of this pass reads
        if (conv_next < need_lo) conv_lo = conv_next = need_lo;
        int conv_end = conv_target > conv_next ? conv_target : conv_next;
        if (need_lo < conv_lo || need_lo < conv_end - 4) {        // the image ring (4 chunks) has moved past it: converted again
          conv_lo = conv_next = need_lo;
          conv_end = conv_target > need_lo ? conv_target : need_lo;
        }
        while (dma_next < conv_end + 2) chunk_dma(dma_next++);
        // records of the two passes behind this one set out now (exact start of the next pass, a guess for the one behind)
        const int jn = j0 + N.nok[0] + N.nok[1];
        rbA = jn >> kRecShift;
        rbB = (jn + 120) >> kRecShift;
        fetch_records((pk + 1) & 3, rbA);
        fetch_records((pk + 2) & 3, rbB);
        __builtin_amdgcn_s_waitcnt(0x0F70);
        wave_lds_fence();
        if (!skip) {
#pragma unroll 1
          while (conv_next < conv_end) {
            if (conv_next >= dma_bad) {
              skip = true;
              break;
            }
            const bool ok = convert_chunk(kPass * conv_next) == 0ull;
            if (!ok) {
              skip = true;
              break;
            }
            ++conv_next;
          }
        }
        if (!skip && conv_next + 1 >= dma_bad) skip = true;      // the loop would convert a chunk that was never fetched
      }
      if (skip) {
        if (!(Q.fl0 & kTileEdge)) push_tile(Ta + (j0 >> 10));
        j0 = tend;
        mode = 0;
        continue;
      }
      // The pass's bank and, unless it is a full pass for the loop, its outputs: one block per regime, so that the four slice-2
      // fragments of regime 3 live in that block alone (selected stage by stage, they stayed live through the other regimes' loops)
      wave_lds_fence();
      const int offs = ws - wbase - 31;
      const bool full = N.nok[1] >= 1 && N.nok[0] + N.nok[1] >= 120;
      auto finish = [&](auto mode_tag) {
        constexpr int MODE = decltype(mode_tag)::value;
        bank_image3m<MODE != 1, MODE == 3>(L, fr, fmr, fsw, offs, l, bank_xv_img(l));
        wave_lds_fence();
        j0 += N.nok[0] + N.nok[1];
        ++pk;
        rbC = (j0 + 240) >> kRecShift;
        if (full) return;
        float res[2];
        out_pass(mode_tag, N, res);
        if constexpr (kTwo) {                     // the other channel through the same rows
          float res1[2];
          wave_lds_fence();
          bank_image3m<MODE != 1, MODE == 3>(L, fr, fmr, fsw, offs, l, bank_xv_img(l), 1);
          wave_lds_fence();
          out_pass(mode_tag, N, res1, 1);
          store_pass2(N, res, res1);
        } else {
          store_pass(N, res);
        }
      };
      // (a full pass leaves with ITS block's regime for the caller to choose the loop by: chosen from `regime` again, the order-6
      // loop could be reached from every block, and its fragments stayed live through all of them)
      if (kMom && regime == 3) {
        fsw_load(true);
        finish(std::integral_constant<int, kMom ? 3 : 1>{});
        if (full) {
          P = N;
          return 3;                               // (the loop's caller puts the folded fragments back)
        }
        fsw_load(false);
      } else if (kMom && regime == 2) {
        finish(std::integral_constant<int, kMom ? 2 : 1>{});
        if (full) {
          P = N;
          return 2;
        }
      } else {
        finish(std::integral_constant<int, 1>{});
        if (full) {
          P = N;
          return 1;
        }
      }
    }
  };

#if PAR_S2_EXP & 64
  unsigned long long s3t_[4] = {0, 0, 0, 0}, s3last_ = __builtin_readcyclecounter();
  const unsigned long long s3start_ = s3last_;
#endif
  // ---- the loop: see the head of this kernel.  Leaves with P finished and j0 at a pass start_run() has to look at.
  auto hot = [&](auto mode_tag) {
    constexpr int MODE = decltype(mode_tag)::value;
    // the lane's image in the folded slice's signal fragment (bank_load): formed here, once per run of the loop -- the order-6 loop
    // has no use for it and no register to carry it in.  (Its value hidden: known to be 0 or one image, the OR behind the ring's
    // mask is compiled as an add of its own.)
    S3XvLane xv_img = {0u, 0u};
    if constexpr (MODE != 3) {
      xv_img = bank_xv_img(l);
      asm volatile("" : "+v"(xv_img.at), "+v"(xv_img.img));
    }
    // (the cold path left the loop's state in vector registers: it is wave-uniform, and stays so through the loop)
    j0 = __builtin_amdgcn_readfirstlane(j0);
    wbase = __builtin_amdgcn_readfirstlane(wbase);
    rbA = __builtin_amdgcn_readfirstlane(rbA);
    rbB = __builtin_amdgcn_readfirstlane(rbB);
    rbC = __builtin_amdgcn_readfirstlane(rbC);
    tc_tend = __builtin_amdgcn_readfirstlane(tc_tend);
    tc_flm = __builtin_amdgcn_readfirstlane(tc_flm);
    // The pass counter, the conversion's chunk and the ring's next chunk advance in lockstep through the loop: ONE carried value,
    // w0 = 128 x conv_next, and fixed differences to it (r09).  What the iteration needs of the three is carried in the form it is
    // used in -- the record buffer as a byte offset, the next chunk's source address and ring slot as running values -- and the
    // limits w0 is compared with are formed here, once per run: conv_next, dma_next and pk are named again where the loop leaves.
    const int cn0 = __builtin_amdgcn_readfirstlane(conv_next), pk0 = __builtin_amdgcn_readfirstlane(pk);
    const int dn0 = __builtin_amdgcn_readfirstlane(dma_next), dbad = __builtin_amdgcn_readfirstlane(dma_bad);
    int w0 = kPass * cn0;
    unsigned rbytes = kRecBufBytes * (unsigned)(pk0 & 3);
    unsigned dslot = kChunkBytes * (unsigned)(dn0 & 7);
    unsigned long long dsrc = ring_src + (unsigned long long)((long long)kChunkBytes * dn0);
    dsrc = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(dsrc >> 32)) << 32) |
           (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)dsrc);
    const int nJm = nJ - kPass;                  // j0 + kPass <= nJ
    const int cn_lim = kPass * (dbad - 2);       // conv_next + 1 < dma_bad (the chunk the NEXT iteration converts was fetched from the file)
    const int dn_lim = kPass * (dbad - (dn0 - cn0));      // dma_next < dma_bad, as a bound on w0
    unsigned long long cok = 0ull;               // the conversion's verdict: zero when the chunk suits float16
    // The loop's exit test is ONE signed margin m, the minimum of a margin per term: the pass stays in the loop while m >= 0
    // (r09: a subtract and a minimum per term where every term was compare -> select -> AND of 64-bit masks).
    int m = 0, adv = 0;                          // (adv: the outputs the placed pass finishes)
    for (;;) {
#if PAR_S2_EXP & 64
      const unsigned long long tA_ = __builtin_readcyclecounter();
#endif
      if constexpr (NCH == 2) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");      // (seven memory operations per iteration)
      else asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
#if PAR_S2_EXP & 64
      const unsigned long long tB_ = __builtin_readcyclecounter();
      s3t_[0] += tB_ - tA_;
      s3t_[1] += tA_ - s3last_;
      s3last_ = tB_;
      s3t_[2] += 1;
#endif
      wave_lds_fence();
      // PLACE(pk): the pass behind P
      S3Pass N;
      int wsK;
      const int jb = (j0 >> kRecShift) - rbA;     // the pass's first block in its record buffer: 0 or 1 where the guess held
      auto place_next = [&](auto early, const PlaceRecs& RR) {
      const Placed Q = place_impl(j0, rbytes, jb, early, RR);
      // The lane tests in two masks: `none` must be empty, `some` must not be.  With ep >= 0 as its bit pattern (epm):
      //   none  a lane outside the record model or on a tie (bad), or too steep for the loop: epm > 2^-24 in the fc = 1 loop (1 + ep
      //         != 1 in float32: a lane with fc < 1), > 0.0105 in the order-5 loop, > 0.0125 (the moment correction's limit)
      //         in the order-6 loop -- each limit lies below the next, so one compare covers the lower ones' terms;
      //   some  the loop's reason to be: a lane with fc < 1 in the order-5 loop, a lane above 0.95 x 0.0105 in the order-6 loop
      //         (no flapping between the two; such a lane has fc < 1).
      constexpr int kEpGen = 0x33800000;          // 2^-24
      const int ep_hi = MODE == 1 ? kEpGen : (MODE == 2 ? __float_as_int(kEpMom5) : __float_as_int(kEpMaxMom));
      const int n_none = __popcll(__ballot(((Q.R[0].m | Q.R[1].m) & kRecBadFlags) != 0u || Q.R[0].tie || Q.R[1].tie || Q.epm > ep_hi));
      int n_some = 1;
      if constexpr (MODE == 2) n_some = __popcll(__ballot(Q.epm > kEpGen));
      if constexpr (MODE == 3) n_some = __popcll(__ballot(Q.epm > __float_as_int(kEpMom5Lo)));
      const int ws = __builtin_amdgcn_readfirstlane(Q.R[0].c) & ~7;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        N.cw[r] = Q.R[r].c - ws;
        N.s[r] = Q.R[r].s;
        N.ep[r] = Q.R[r].ep;
        N.nok[r] = __popcll(__ballot(N.cw[r] < kPass));
      }
      N.j = j0;
      N.ws = ws;
      wsK = ws - wbase;
      const int d = w0 - wsK;                     // image converted up to d samples beyond the first bank centre
      // neither tile flagged; the whole pass inside the range; >= 120 finished outputs (which imply a full first row);
      // 161 <= d <= 473; the next chunk to convert came from the file; the records' guess held
      // (the masks enter as lane COUNTS: a select on `mask == 0` is compiled as 64-bit mask algebra and a vector select.  A pass
      // finishes <= 128 outputs, so 16 x n_none sinks that margin below zero whatever the pass finishes)
      // (every term is wave-uniform, and every minimum is pinned to a scalar register where it is formed -- no instruction: left
      // alone the compiler folds min(min(a, b), c) into min3, which only the vector unit has, and the chain's tail ran there from
      // copies of its scalar terms, r10)
      auto smin = [](int x, int y) {
        int r = min(x, y);
        asm volatile("" : "+s"(r));
        return r;
      };
      adv = N.nok[0] + N.nok[1];
      m = smin(tc_flm, nJm - j0);
      m = smin(m, adv - 120 - 16 * n_none);
      m = smin(m, smin(d - 161, 473 - d));
      m = smin(m, cn_lim - w0);
      m = smin(m, smin(jb, 1 - jb));
      if constexpr (MODE != 1) m = smin(m, n_some - 1);
      };
      float res[2];
      if constexpr (kEarly) {
        // The mono loop, every LDS read issued a stage ahead of its use (the order at the head of this kernel).  The reads whose
        // addresses the loop's state names: the records of PLACE(pk), the conversion's chunk, the gathers of OUT(P)
        const PlaceRecs RR = place_load(j0, rbytes, jb);
        const float2 cxx = s3_convert_load(L, w0, l);
        S3Gather G[2];
        const int wsP = P.ws - wbase;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          int ci = P.cw[r];
          ci = ci < 0 ? 0 : (ci > kPass - 1 ? kPass - 1 : ci);
          G[r] = s3_out_load<MODE, NCH>(L, ci, wsP);
        }
        __builtin_amdgcn_sched_barrier(0);
        // PLACE(pk) waits for the records alone; the chunk and the gathers land under it
        place_next(std::true_type{}, RR);
        // BANK(pk)'s image fragments set out as soon as ws is known ...
        const S3Frags X = bank_load<MODE != 3, MODE != 1>(L, wsK - 31, l, xv_img);
        __builtin_amdgcn_sched_barrier(0);
        // ... and OUT(P)'s arithmetic runs while they are on their way.  (Pinned: left alone the compiler sinks a row's arithmetic
        // into its store's lane mask at the END of the iteration, as in the stereo loop.)
        if constexpr (MODE == 2) {
          // Order 5: OUT(P)'s first row in the fragments' shadow, its second row left to the matrix work -- an MFMA hides two
          // vector instructions behind it, so the row is dealt out two to an MFMA for as long as it lasts.  (Not the
          // order-6 loop: with 31 MFMAs and nine accumulators live the scheduler does not take the pipeline and leaves the whole
          // row behind the first MFMA.  Not the fc = 1 loop: its rows are short, and with one of them gone the first fragment
          // is waited for 84 priced cycles after its read instead of 167; measured, the step is the same either way, NOTES r08.)
          res[0] = s3_out_math<MODE>(G[0], P.s[0], P.ep[0]);
          asm volatile("" : "+v"(res[0]));
          // (order 5 leaves m6 of the gathered rows unread: kept alive to here, or its register is handed out again under
          // PLACE and the write to it waits for the LAST gather)
          asm volatile("" ::"v"(G[0].Mh[3]));
          __builtin_amdgcn_sched_barrier(0);
          // the matrix work and the row writes (behind OUT(P)'s gathers)
          res[1] = s3_out_math<MODE>(G[1], P.s[1], P.ep[1]);
          bank_math<true, false>(L, fr, fmr, fsw, X, l);
          asm volatile("" : "+v"(res[1]));
          asm volatile("" ::"v"(G[1].Mh[3]));
#pragma unroll
          for (int i = 0; i < 24; ++i) {                            // (the bank's 11 + 13 MFMAs)
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // one MFMA
            __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);      // two VALU
          }
        } else {
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            res[r] = s3_out_math<MODE>(G[r], P.s[r], P.ep[r]);
            // (order 6: one row after the other -- interleaved, the rows' temporaries are the kernel's register peak)
            if constexpr (MODE == 3) {
              asm volatile("" : "+v"(res[r]));
              __builtin_amdgcn_sched_barrier(0);
            }
          }
          asm volatile("" : "+v"(res[0]), "+v"(res[1]));
          __builtin_amdgcn_sched_barrier(0);
          // the matrix work and the row writes (behind OUT(P)'s gathers)
          bank_math<MODE != 1, MODE == 3>(L, fr, fmr, fsw, X, l);
        }
        // CONV's arithmetic and image writes (behind the fragment reads), then FETCH and the stores: five memory operations, in
        // this order.  (The loop's exit margin is scalar work since r10 -- formed in place_next, min by min -- and needs no place
        // beside the matrix work: until then its tail ran on the vector port and was pinned here.)
        cok = s3_convert_math(L, w0, l, cxx);
        fetch_records_at(rbytes ^ (2 * kRecBufBytes), rbC);
        chunk_dma_at(w0 < dn_lim, dsrc, dslot);
        store_pass(P, res);
      } else {
      if constexpr (!kTwo) place_next(std::false_type{}, PlaceRecs{});      // (stereo: behind OUT(P, 1), fewer registers live through the banks)
      // BANK(pk) over [ws, ws + 128): image samples converted in earlier iterations
      // OUT(P) first in program order: its gathers must precede the bank's row writes
      out_pass(mode_tag, P, res);
      if constexpr (kTwo) {
        // Stereo.  The bank rows in LDS hold ONE channel of one pass at a time: on entry channel 0 of P (banked by the previous
        // iteration or by the cold path).  OUT(P, 0) above has gathered them; now BANK(P, 1) -> OUT(P, 1) -> BANK(N, 0), each after
        // the reads of what it overwrites in program order.  Channel 1's image therefore runs one chunk behind channel 0's: its
        // bank of a pass sees the image exactly as channel 0's bank of that pass did one iteration earlier.
        float res1[2];
        // (pinned here: left alone the compiler sinks a row's arithmetic into the store's lane mask at the END of the iteration,
        // and the gathered rows and ring samples of both channels stay live through the banks: 33 registers in scratch)
        asm volatile("" : "+v"(res[0]), "+v"(res[1]));
        bank_image3m<MODE != 1, MODE == 3>(L, fr, fmr, fsw, P.ws - wbase - 31, l, xv_img, 1);
        out_pass(mode_tag, P, res1, 1);
        asm volatile("" : "+v"(res1[0]), "+v"(res1[1]));
        place_next(std::false_type{}, PlaceRecs{});
        const int offs = wsK - 31;
        bank_image3m<MODE != 1, MODE == 3>(L, fr, fmr, fsw, offs, l, xv_img, 0);
        const unsigned long long c0 = s3_convert_ch(L, w0, l, 0, true);
        const unsigned long long c1 = s3_convert_ch(L, w0 - kPass, l, 1, false);
        cok = c0 | c1;
        fetch_records_at(rbytes ^ (2 * kRecBufBytes), rbC);
        chunk_dma_at(w0 < dn_lim, dsrc, dslot);
        store_pass2(P, res, res1);
      } else {
        const int offs = wsK - 31;
#if PAR_S3_PIN_MONO
        asm volatile("" : "+v"(res[0]), "+v"(res[1]));
#endif
        bank_image3m<MODE != 1, MODE == 3>(L, fr, fmr, fsw, offs, l, xv_img);
        // CONV: one chunk per iteration
        cok = convert_chunk(w0);
        // FETCH + stores: records of pass pk + 2, chunk conv_next + 2, then P's outputs (five memory operations, in this order)
        fetch_records_at(rbytes ^ (2 * kRecBufBytes), rbC);
        chunk_dma_at(w0 < dn_lim, dsrc, dslot);
        store_pass(P, res);
      }
      }
      wave_lds_fence();
      w0 += kPass;
      dsrc += kChunkBytes;
      dslot = (dslot + kChunkBytes) & (8 * kChunkBytes - 1);
      S3_COUNT(2);
      if (min(m, -(int)__popcll(cok)) < 0) break;
      // N becomes P
      P = N;
      j0 += adv;
      rbytes = (rbytes + kRecBufBytes) & (3 * kRecBufBytes);
      rbA = rbB;
      rbB = rbC;
      rbC = (j0 + 240) >> kRecShift;
    }
    conv_next = w0 >> 7;                          // (the pass that left the loop converted its chunk and was not counted)
    dma_next = dn0 + (conv_next - cn0);
    pk = pk0 + (conv_next - cn0) - 1;
    if (cok != 0ull) mode = 0;                    // (start_run converts again and sends the tile to the block kernel)
    // stereo: channel 1's image catches up with channel 0's before the cold path takes over
    if constexpr (kTwo)
      if (mode != 0 && s3_convert_ch(L, w0 - kPass, l, 1, false) != 0ull) mode = 0;
  };

  while (const int run = start_run()) {
    if (kMom && run == 3) {
      hot(std::integral_constant<int, kMom ? 3 : 1>{});
      fsw_load(false);
    } else if (kMom && run == 2) hot(std::integral_constant<int, kMom ? 2 : 1>{});
    else hot(std::integral_constant<int, 1>{});
    // P has been finished by the loop; the pass at j0 needs the cold path
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);
#if PAR_S2_EXP & 64
  if (l == 0) {
    unsigned long long* o = g_s2_phase + (size_t)stream_id * 16;
    o[0] = s3t_[0];                                // cycles in the loop's memory wait (includes two clock reads)
    o[1] = s3t_[1];                                // cycles between the end of one wait and the start of the next
    o[2] = s3t_[2];                                // iterations
    o[3] = __builtin_readcyclecounter() - s3start_;      // the wave's whole life behind its set-up
    o[6] = s3t_[2];
  }
#endif
}

template <int NCH, int KIND>
__global__ __launch_bounds__(kWave, KIND == 1 ? 3 : 2) void k_sinc_pipe(const S2Args a) {
  __shared__ S3Lds<NCH, KIND != 1> L;
  sinc_pipe_body<NCH, KIND>(a, (int)blockIdx.x, L);
}

// Several files in ONE launch (r06; the archive's 10-min files): a file's K_sinc is two or three kernels, each with a tail in
// which the GPU empties, plus the gaps between them -- ~0.13 ms per file, a sixth of a 10-min mono file's time.  Here the
// workgroups of file k + 1 follow those of file k inside the same grid: the tails and gaps are paid once per launch.
constexpr int kBatchFiles = kFusedBatchMax;
struct S2Batch {
  int n;
  int first[kBatchFiles + 1];                    // first workgroup of file k; first[n] = the grid
  S2Args f[kBatchFiles];
};
static_assert(sizeof(S2Batch) <= 3584, "kernel arguments fit the 4 KB segment");
template <int NCH, int KIND>
__global__ __launch_bounds__(kWave, KIND == 1 ? 3 : 2) void k_sinc_pipe_n(const S2Batch b) {
  __shared__ S3Lds<NCH, KIND != 1> L;
  const int bx = (int)blockIdx.x;
  int fi = 0;
#pragma unroll
  for (int k = 1; k < kBatchFiles; ++k) fi += (k < b.n && bx >= b.first[k]) ? 1 : 0;
  const S2Args* pa = &b.f[fi];                    // (kernel-argument memory: scalar loads at a wave-uniform offset)
  const S2Args a = *pa;
  sinc_pipe_body<NCH, KIND>(a, bx - b.first[fi], L);
}

// wave slots of the device for the two-waves-per-SIMD kernels (compute units x 4 SIMDs x 2; 2 048 on an MI355X): from the device's
// properties, so that a partitioned or CU-masked device cuts its streams for what it has
static int64_t stream_wave_slots(int device) {
  static std::atomic<int> cached[64];
  const int d = device >= 0 && device < 64 ? device : 0;
  int v = cached[d].load(std::memory_order_relaxed);
  if (v == 0) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
    v = cus * 8;
    cached[d].store(v, std::memory_order_relaxed);
  }
  return v;
}

// the launch's arguments and its grid for one file
static int64_t make_stream_args(int device, const SincFile& f, const float4* tab, const TapModes& tmd, int64_t pick_out_stride, S2Args& a) {
  const int64_t slots = stream_wave_slots(device);
  const int64_t len_out = f.len_out;
  const FusedArgs& fa = f.fa;
  a.out_stride = pick_out_stride;
  a.len_out = len_out;
  a.sig = f.sig;
  a.len_in = f.len_in;
  a.out = f.out;
  a.hdr = fa.hdr;
  a.rec = fa.rec;
  a.rec2 = fa.rec2;
  a.redo_count = fa.redo_count;
  a.redo_list = fa.redo_list;
  a.fa = fa;
  a.tab = tab;
  a.tmd = tmd;
  a.n_full = len_out / kSincTileOutputs;
  a.n_tiles = ceil_div(len_out, kSincTileOutputs);
  // (launch_sinc_fused only comes here with >= 4 full tiles: the end tiles are distinct)
  a.n_edge = a.n_full >= 4 ? (int)(3 + (a.n_tiles - a.n_full)) * kEdgeWavesPerTile : 0;
  // Tiles per wave of the pipelined kernel: long streams amortise a wave's cold start and, beside a batch driver's plan kernels,
  // leave fewer wave boundaries for them to slip into -- 60-min file, ms per pipelined step: 4 tiles 5.03, 8: 4.84, 12: 4.70,
  // 16: 4.66, 24: 4.61, 32: 5.06 (10.3 rounds of the 2 048 wave slots: the last one nearly empty), 48: 4.67 (r05) -- while a
  // short file still has to fill the GPU's wave slots a few times over.
#ifdef PAR_EXPERIMENT            // (experiment builds only: the product reads no knob from the environment)
  static const int tiles_env = getenv("PAR_S2_TILES_RT") ? std::min(48, std::max(0, atoi(getenv("PAR_S2_TILES_RT")))) : 0;
  static const int tail_env = getenv("PAR_S2_TAIL") ? std::max(0, atoi(getenv("PAR_S2_TAIL"))) : 6;
  static const int tail_rounds = getenv("PAR_S2_TAIL_ROUNDS") ? std::max(0, atoi(getenv("PAR_S2_TAIL_ROUNDS"))) : 1;
#else
  constexpr int tiles_env = 0, tail_env = 6, tail_rounds = 1;      // tail_env: divisor of the last round's stream length
#endif
  const int64_t want = a.n_full / (4 * slots);
  // ... and an ODD number of them (r06): the concurrent streams start tiles x 4 KB (8 KB stereo) apart, and when that is a multiple
  // of 64 KB they camp on the same memory channels -- 60-min file, ms per step: 32 tiles 5.71, 16: 4.20, 48: 4.19 against
  // 4.09-4.18 for every odd count from 17 to 37 and 4.02-4.19 for 24 (what looked like rounds of the wave slots in r05 was this)
  a.tiles = tiles_env > 0 ? tiles_env : (int)(want < 8 ? 8 : (want > kMaxTilesPerWave ? kMaxTilesPerWave : want)) | 1;
  if (a.tiles > 48) a.tiles = 47;
  // ... and the launch's last round (2 048 wave slots' worth of tiles) as four rounds of quarter-length streams: the tail in which
  // the GPU empties behind the last long streams shrinks with them
  // (24 tiles, K_sinc alone: no short tail 4.37 ms, quarter-length 4.22, 1/8 4.20, 1/12 4.23; two rounds of them 4.23 / 4.30)
  a.tiles_tail = a.tiles >= 8 && tail_env > 1 ? std::max(2, a.tiles / tail_env) | 1 : a.tiles;
  a.n_big = (a.n_full - std::min<int64_t>(a.n_full, slots * tail_rounds * a.tiles * (a.tiles_tail < a.tiles ? 1 : 0))) / a.tiles;
  return a.n_big + ceil_div(a.n_full - a.n_big * a.tiles, (int64_t)a.tiles_tail) + a.n_edge;
}

int launch_sinc_stream(int device, SincRoute route, const SincFile& f, int64_t pick_out_stride, const float4* tab, const TapModes& tmd,
                       hipStream_t s) {
  S2Args a;
  const int64_t grid = make_stream_args(device, f, tab, tmd, route == SincRoute::StreamPick ? pick_out_stride : 0, a);
  const dim3 g((unsigned)grid), b(kWave);
  if (route == SincRoute::Block) return PAR_ERR_ARG;
  if (grid > 0) {
    switch (route) {
      case SincRoute::StreamPick: hipLaunchKernelGGL((k_sinc_pipe<2, 3>), g, b, 0, s, a); break;
      case SincRoute::StreamStereo: hipLaunchKernelGGL((k_sinc_pipe<2, 0>), g, b, 0, s, a); break;
      default:
        // mono: the streams with an fc < 1 tile (two waves per SIMD: all 25 constant fragments) and the end tiles, then the fc = 1
        // streams (three per SIMD), over the same grid -- a wave of the other kind leaves behind its tile headers
        hipLaunchKernelGGL((k_sinc_pipe<1, 2>), g, b, 0, s, a);
        hipLaunchKernelGGL((k_sinc_pipe<1, 1>), g, b, 0, s, a);
    }
  }
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}

// n <= kBatchFiles files of ONE route (StreamMono or StreamStereo) in one launch per kernel kind
int launch_sinc_stream_batch(int device, SincRoute route, int n, const SincFile* files, const float4* tab, const TapModes& tmd, hipStream_t s) {
  if (n < 1 || n > kBatchFiles) return PAR_ERR_ARG;
  S2Batch b;
  b.n = n;
  int64_t at = 0;
  for (int k = 0; k < n; ++k) {
    b.first[k] = (int)at;
    at += make_stream_args(device, files[k], tab, tmd, 0, b.f[k]);
    if (at > INT_MAX) return PAR_ERR_ARG;
  }
  for (int k = n; k <= kBatchFiles; ++k) b.first[k] = (int)at;
  if (at <= 0) return PAR_OK;
  const dim3 g((unsigned)at), w(kWave);
  switch (route) {
    case SincRoute::StreamStereo: hipLaunchKernelGGL((k_sinc_pipe_n<2, 0>), g, w, 0, s, b); break;
    case SincRoute::StreamMono:
      hipLaunchKernelGGL((k_sinc_pipe_n<1, 2>), g, w, 0, s, b);
      hipLaunchKernelGGL((k_sinc_pipe_n<1, 1>), g, w, 0, s, b);
      break;
    default: return PAR_ERR_ARG;          // (StreamPick never merges)
  }
  PAR_HIP_CHECK(hipGetLastError());
  return PAR_OK;
}

}  // namespace par

#if PAR_S2_EXP & 64
extern "C" int par_debug_s2_phase_buffer(unsigned long long* dev_buf) {
  return hipMemcpyToSymbol(HIP_SYMBOL(par::g_s2_phase), &dev_buf, sizeof(dev_buf)) == hipSuccess ? 0 : 1;
}
#endif
