/*
 * crtfx_signal.h — the composite-video stage of libcrtfx.so: every row of an h x w x 3 RGB frame (CRTFX_PIX_U8 or CRTFX_PIX_F16) is encoded
 * to an NTSC-like signal and decoded again on the device — the cable that fed the tube: colour that bleeds sideways, dot crawl on colour
 * edges, rainbow fringes on fine luma detail.  One pixel is one sample at four times the colour subcarrier (an active NTSC line is about
 * 754 such samples), so the stage stands at the SOURCE's size, directly behind the source plan and in front of the deinterlacer, the Canvas
 * and the resize (pythoncrt_amd/signal.py, ends.py).  At that rate the subcarrier's cosine and sine take only the values
 * {1, 0, -1, 0}: the whole cascade is integer arithmetic.
 *
 * Status codes (crtfx_status), pixel formats (crtfx_pixfmt) and conventions are those of crtfx.h: the caller owns every frame; work is
 * enqueued on the caller's hipStream_t (void*, NULL = the default stream); only destroy synchronises; the calling thread's current device
 * must be the plan's when it runs.  The stage depends on a device and six numbers, not on a crtfx_ctx: it has a handle of its own, the
 * handle owns no device memory, and it keeps nothing from one run to the next (the frame index is an argument of every run).
 *
 * Arithmetic, bit for bit; this is the library's own rule (tests/signal_model.py restates it in numpy, tests/test_signal_tables.py and
 * test_signal_gpu.py hold the kernels to it with no differing element).  NOT claimed is equality with any other NTSC implementation.
 * Codes: the codes 0..255 of uint8 frames; of half frames the quarter codes q = rint_to_even(min(max(4 f, 0), 1020)), NaN -> 0 (the
 * quantiser of crtfx_resize16.h), and a result r is written as half(r / 4), which is exact.  M is 255 for uint8 and 1020 for half.  Every
 * output sample is computed: there is no bit-keeping mode.  Every >> is an arithmetic shift: a floor.
 * Rows are independent.  A row is extended to both sides by its edge pixels (R, G and B replicated), and every quantity below is defined
 * on the extended row at every integer x, x < 0 and x >= w included; the phase uses the true x.
 *     phase     p(x, y, t) = (x + 2 y + 2 c t) mod 4, taken non-negative: y the row, t the frame's index in the stream, c = 1 with crawl
 *               and 0 without; cos[p] = {1, 0, -1, 0}, sin[p] = {0, 1, 0, -1}: 180 degrees per line and per frame
 *     step 1    Y0 = (1225 R + 2404 G +  467 B + 128) >> 8        (16 per code)
 *               I0 = (2441 R - 1125 G - 1316 B + 128) >> 8
 *               Q0 = ( 866 R - 2141 G + 1275 B + 128) >> 8
 *     step 2    T7 = [1 2 3 4 3 2 1] (sum 16): I1(x) = (sum_k T7[k] I0(x + k) + 8) >> 4, k = -3..3; Q1 from Q0 the same way
 *     step 3    C(x) = I1(x) cos[p] + Q1(x) sin[p]                 (one of I1, -I1, Q1, -Q1)
 *     step 4    CRTFX_SIGNAL_COMPOSITE: s = Y0 + C, not clipped; Yd(x) = (s(x - 2) + 2 s(x) + s(x + 2) + 2) >> 2 (a notch at the
 *               subcarrier); e = s - Yd
 *               CRTFX_SIGNAL_SVIDEO: Yd = Y0, e = C: no crosstalk, and the result depends on neither the line nor the frame phase, so
 *               crawl changes nothing
 *     step 5    Id0(x) = 2 e(x) cos[p], Qd0(x) = 2 e(x) sin[p]
 *     step 6    CRTFX_SIGNAL_SHARP: D = T7, shift 4; CRTFX_SIGNAL_SOFT: D = T15 = [1 2 .. 8 .. 2 1] (sum 64), shift 6, r = 3 or 7:
 *               Id(x) = (sum_k D[k] Id0(x + k) + (1 << (shift - 1))) >> shift, k = -r..r; Qd from Qd0 the same way
 *     step 7    R = (4096 Yd + 3916 Id + 2543 Qd + 32768) >> 16
 *               G = (4096 Yd - 1114 Id - 2651 Qd + 32768) >> 16
 *               B = (4096 Yd - 4533 Id + 6981 Qd + 32768) >> 16, each clamped to 0..M
 * A result reaches 3 + 2 + 3 = 8 pixels to either side under SHARP and 12 under SOFT (6 and 10 under SVIDEO).  Y0, I0, Q0, I1, Q1, s and
 * Yd fit int16: on quarter codes |I0| <= 9726, |Q0| <= 8531 and s lies within -9726 .. 26046.  Every accumulator fits int32; by the sum
 * of absolute values the last one stays below 9.3e8.  A flat colour returns itself (T7 and T15 average the 4-periodic carrier exactly), and
 * so does any grey frame under SVIDEO.
 *
 * Frames: 3 bytes per pixel (uint8) or 6 (half), rows unpadded; the same size and sample type go in and out, one output frame per source
 * frame.  For half frames every frame base and frame stride must be even (CRTFX_E_INVALID otherwise); uint8 frames may start anywhere.
 *
 * Stated limits: NTSC-like only — no PAL, no burst-axis rotation, no RF noise.  The rows of a woven interlaced frame are taken as
 * consecutive lines.  The chroma rows of a 4:2:0 source are formed in front of this stage by its source plan.
 *
 * Paths; both give the same bytes, the path is chosen per run, and *_last_plan names the one that ran.  Sixteen builds.
 * k_signal<signal,chroma,pix,vec>: runs where
 *     w % 8 == 0, both frame bases are multiples of 4, and so are both strides where n > 1
 * — the rule of crtfx_deint.h.  One wave takes a segment of 488 pixels of one row of one frame (with the halo of 12 to either side that is
 * 512 = 64 lanes x 8), four waves a workgroup, all frames of a launch one grid (grid.z; 32768 frames per launch).  The cascade is staged
 * through four int16 planes of the wave's own in LDS: a lane loads 8 pixels of segment and halo as two dword-multiple loads at
 * dword-aligned addresses (a group of four pixels lies inside the row or outside it; one outside is the edge pixel), quantises halves two
 * at a time and writes Y0 / I0 / Q0 as three 16-byte LDS stores; behind a barrier it reads 16 entries of each plane as 16-byte loads,
 * forms 8 samples of s (of C under SVIDEO) — the phase of a sample is a constant of its place in the lane's eight, turned by 180
 * degrees per row and frame, so the carrier products are selections, and only the one of I1 / Q1 that the phase keeps is formed — and
 * writes them as one 16-byte store; behind a second barrier the lane that owns 8 output pixels reads 24 (SHARP) or 32 (SOFT) entries of s,
 * forms e, the demodulated products and both D sums in registers (the half of the taps whose carrier factor is zero is left out), runs
 * the matrix and stores its 24 results as dword-multiples.  Consecutive lanes touch consecutive 16 bytes of LDS at every step.
 * k_signal<signal,chroma,pix,general>: any size and alignment, and the CRTFX_SIGNAL_OPT_FORCE_GENERAL fallback: one lane per pixel
 * evaluates the cascade of that pixel from 17 (SHARP) or 25 (SOFT) pixels loaded at clamped columns, 1-byte (2-byte) loads and stores;
 * grid = (pixels of a row, rows, frames).
 * Every output element is written by exactly one lane on either path; column indices are clamped, not padded, so no byte outside a source
 * frame is read; bytes between frames are neither read nor written.
 *
 * Registers (gfx950, as built; tests/test_signal_tables.py reads them from the library): VGPRs of k_signal<signal,chroma,pix,path>
 *     k_signal<composite,sharp,u8,vec> 50, k_signal<composite,sharp,f16,vec> 49, k_signal<composite,soft,u8,vec> 57, k_signal<composite,soft,f16,vec> 53,
 *     k_signal<svideo,sharp,u8,vec> 50, k_signal<svideo,sharp,f16,vec> 41, k_signal<svideo,soft,u8,vec> 56, k_signal<svideo,soft,f16,vec> 50,
 *     k_signal<composite,sharp,u8,general> 59, k_signal<composite,sharp,f16,general> 59, k_signal<composite,soft,u8,general> 83, k_signal<composite,soft,f16,general> 83,
 *     k_signal<svideo,sharp,u8,general> 45, k_signal<svideo,sharp,f16,general> 45, k_signal<svideo,soft,u8,general> 60, k_signal<svideo,soft,f16,general> 60
 * (eight waves per SIMD for every build but the general SOFT composite ones, which hold the 25 pixels' Y / I / Q at once and run five);
 * LDS: 16896 bytes per workgroup for every vec build (4 waves x 4 planes x 528 int16), none for the general ones;
 * no AGPRs, no scratch, no spills.
 *
 * Kernel time per frame: measured once on one MI355X in batches of 8 (tools/signal_kernel_times.py, HIP events, launch gaps included;
 * profiles/signal.txt holds the whole output), next to a device-to-device copy of equal traffic (one frame read, one written) and the
 * untouched k_deint<edge,pix,first,vec> (the same traffic), all timed in the same run; us, vec / general / copy / k_deint:
 *                                      uint8                            half
 *     480 x 720    composite, sharp    1.60 /  8.63 / 0.39 / 1.75       2.06 /  9.99 / 0.52 / 2.54
 *                  composite, soft     1.73 / 12.87 / 0.44 / 1.71       2.18 / 14.61 / 0.51 / 2.47
 *                  svideo, sharp       1.39 /  5.30 / 0.41 / 1.71       1.79 /  6.48 / 0.51 / 2.47
 *                  svideo, soft        1.52 /  9.26 / 0.40 / 1.71       1.92 / 10.89 / 0.51 / 2.47
 *     1080 x 1920  composite, sharp    5.36 / 46.14 / 1.59 / 5.89       7.01 / 53.34 / 2.93 / 8.63
 *                  composite, soft     6.28 / 75.21 / 1.60 / 5.90       7.97 / 84.48 / 2.93 / 8.62
 *                  svideo, sharp       4.77 / 30.37 / 1.59 / 5.89       6.35 / 36.30 / 2.93 / 8.60
 *                  svideo, soft        5.36 / 52.52 / 1.59 / 5.90       6.90 / 62.54 / 2.93 / 8.62
 * Eight frames of either size lie in the Infinity Cache, so the copy runs at 4.7 - 8.5 TB/s and is a hard yardstick: the vec path takes
 * 2.2 - 4.3 x the copy — it is bound by its arithmetic and its two trips through LDS, not by memory — and 0.74 - 1.06 x k_deint's EDGE, a
 * stage of the same traffic with a search per pixel.  The general path takes 3.6 - 7.4 x the vec path at 480 x 720 and 5.7 - 12.0 x at
 * 1080 x 1920: vec is the faster path at both sizes for every build, so vec runs whenever its conditions hold.
 */
#ifndef CRTFX_SIGNAL_H
#define CRTFX_SIGNAL_H

#include <stddef.h>
#include <stdint.h>

#include "crtfx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crtfx_signal crtfx_signal;

typedef enum crtfx_signal_kind { CRTFX_SIGNAL_COMPOSITE = 0, CRTFX_SIGNAL_SVIDEO = 1 } crtfx_signal_kind;
typedef enum crtfx_signal_chroma { CRTFX_SIGNAL_SHARP = 0, CRTFX_SIGNAL_SOFT = 1 } crtfx_signal_chroma;

/* Plans the stage for h x w x 3 frames of pix_fmt (CRTFX_PIX_U8 or CRTFX_PIX_F16) on `device` (the calling thread's current device is
 * restored).  crawl is 0 or 1.  CRTFX_E_INVALID: a null out pointer, h or w < 1 or > 32767, an unknown pix_fmt, signal or chroma, a crawl
 * that is neither 0 nor 1.  All of these are refused before a device is touched.  When it fails *out_plan is NULL and
 * crtfx_signal_last_error(NULL) holds the message (per calling thread), which names the offending field. */
int crtfx_signal_create(int device, int h, int w, int pix_fmt, int signal, int chroma, int crawl, crtfx_signal** out_plan);
int crtfx_signal_destroy(crtfx_signal* plan);
const char* crtfx_signal_last_error(const crtfx_signal* plan);

/* n frames in one call: frame i is read at src_base + i * src_stride_bytes and written at dst_base + i * dst_stride_bytes (h x w x 3
 * samples each, rows unpadded), and its t is first_index + i, of which only the parity matters.  n = 0 does nothing.  CRTFX_E_INVALID: a
 * negative first_index, n < 0, a null frame pointer, a stride shorter than a frame (n > 1), an odd base or stride for half frames, and a
 * source range [src_base, src_base + (n - 1) * stride + frame) that overlaps the destination's.  Bytes between frames are neither read
 * nor written. */
int crtfx_signal_run(crtfx_signal* plan, int64_t first_index, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes,
                     int n, void* stream);

/* Testing / A-B switches of one plan.  FORCE_GENERAL (0 / 1): take the general kernel whatever the width and alignment. */
typedef enum crtfx_signal_option { CRTFX_SIGNAL_OPT_FORCE_GENERAL = 1 } crtfx_signal_option;
int crtfx_signal_set_option(crtfx_signal* plan, int option, int value);

/* The path of the most recent crtfx_signal_run (before the first one: the path a run with aligned frames takes) and its frames:
 * `signal=k_signal<composite,soft,u8,vec>;frames=5` or `signal=k_signal<svideo,sharp,f16,general>;frames=1`. */
int crtfx_signal_last_plan(crtfx_signal* plan, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* CRTFX_SIGNAL_H */
