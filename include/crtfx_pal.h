/*
 * crtfx_pal.h — the PAL composite-video stage of libcrtfx.so: every row of an h x w x 3 RGB frame (CRTFX_PIX_U8 or CRTFX_PIX_F16) is encoded
 * to a PAL-like signal and decoded again on the device, by a decoder with a phase error and — CRTFX_PAL_DELAY — a one-line delay line: the
 * cable of 576i sources.  The subcarrier turns 270 degrees per line and per frame, the V axis switches sign every line, and the decoder
 * averages each line's chroma with the line before: a phase error then desaturates the picture instead of turning its hue, and vertical
 * chroma detail is halved.  Without the delay line (CRTFX_PAL_SIMPLE) a phase error shows as Hanover bars.  One pixel is one sample at four
 * times the colour subcarrier, so the stage stands at the SOURCE's size, where the NTSC stage stands (crtfx_signal.h, whose family is
 * untouched and has no phase knob; pythoncrt_amd/pal.py, ends.py).  The whole cascade is integer arithmetic.
 *
 * Status codes (crtfx_status), pixel formats (crtfx_pixfmt) and conventions are those of crtfx.h: the caller owns every frame; work is
 * enqueued on the caller's hipStream_t (void*, NULL = the default stream); only destroy synchronises; the calling thread's current device
 * must be the plan's when it runs.  The stage depends on a device and eight numbers, not on a crtfx_ctx: it has a handle of its own, the
 * handle owns no device memory, and it keeps nothing from one run to the next (the frame index is an argument of every run).
 *
 * Arithmetic, bit for bit; this is the library's own rule (tests/pal_model.py restates it in numpy, tests/test_pal_tables.py and
 * test_pal_gpu.py hold the kernels to it with no differing element).  NOT claimed is equality with any other PAL implementation.
 * Codes, M, the half quantiser, the extension of a row by its edge pixels, T7 / T15, "every >> is a floor" and cos[p] = {1, 0, -1, 0},
 * sin[p] = {0, 1, 0, -1} are those of crtfx_signal.h.  Rows are independent up to step 7.
 *     phase     p(x, y, t) = (x + 3 y + 3 c t) mod 4, taken non-negative: y the row, t the frame's index in the stream, c = 1 with crawl
 *               and 0 without: 270 degrees per line and per frame, so only t mod 4 matters
 *     V switch  v(y, t) = +1 where y + c t is even, -1 otherwise
 *     step 1    Y0 = (1225 R + 2404 G +  467 B + 128) >> 8        (16 per code)
 *               U0 = (-603 R - 1183 G + 1786 B + 128) >> 8
 *               V0 = (2518 R - 2109 G -  409 B + 128) >> 8
 *     step 2    U1(x) = (sum_k T7[k] U0(x + k) + 8) >> 4, k = -3..3; V1 from V0 the same way
 *     step 3    C(x) = U1(x) sin[p] + v V1(x) cos[p]               (one of U1, -U1, V1, -V1)
 *     step 4    CRTFX_PAL_COMPOSITE: s = Y0 + C, not clipped; Yd(x) = (s(x - 2) + 2 s(x) + s(x + 2) + 2) >> 2; e = s - Yd
 *               CRTFX_PAL_SVIDEO: Yd = Y0, e = C
 *     step 5    Ud0(x) = 2 e(x) sin[p], Vd0(x) = 2 e(x) v cos[p]
 *     step 6    CRTFX_PAL_SHARP: D = T7, shift 4; CRTFX_PAL_SOFT: D = T15, shift 6, r = 3 or 7:
 *               Ud(x) = (sum_k D[k] Ud0(x + k) + (1 << (shift - 1))) >> shift, k = -r..r; Vd from Vd0 the same way
 *     step 7    the decoder's phase error theta = `phase` whole degrees, -180..180; the host computes
 *               (c_theta, s_theta) = (llrint(4096 cos theta), llrint(4096 sin theta)) in double (crtfx_pal_phase_table):
 *               Ur = (c_theta Ud + v s_theta Vd + 2048) >> 12
 *               Vr = (c_theta Vd - v s_theta Ud + 2048) >> 12       (the identity at theta = 0)
 *     step 8    CRTFX_PAL_DELAY: the partner row y' is y - 1 for y >= 1; for y = 0 it is row 1, or row 0 itself where h = 1:
 *               U = (Ur(y) + Ur(y') + 1) >> 1, V = (Vr(y) + Vr(y') + 1) >> 1, each row taken with its own p and v, so the s_theta
 *               terms of the two lines cancel
 *               CRTFX_PAL_SIMPLE: U = Ur, V = Vr
 *     step 9    R = (4096 Yd + 4670 V + 32768) >> 16
 *               G = (4096 Yd - 1617 U - 2379 V + 32768) >> 16
 *               B = (4096 Yd + 8325 U + 32768) >> 16, each clamped to 0..M
 * A result reaches 8 pixels to either side under SHARP and 12 under SOFT, and under DELAY one row up (row 0: one row down).  Y0, U0, V0, U1,
 * V1, s and Yd fit int16: on quarter codes |U0| <= 7116, |V0| <= 10033 and s lies within -10033 .. 26353.  Every accumulator fits int32, by
 * the sum of absolute values: |e| <= 36386, so |Ud|, |Vd| <= 36387 (the taps at every other sample sum to half the filter); |c_theta| +
 * |s_theta| <= 5792 (at 45 degrees), so the rotation's accumulators stay below 2.2e8 and |Ur|, |Vr|, |U|, |V| <= 51453; the last accumulator
 * stays below 5.4e8.  At theta = 0 a flat colour returns itself under both signals, both filters and both decoders, and the two matrices
 * return every byte triple exactly.
 *
 * Frames: 3 bytes per pixel (uint8) or 6 (half), rows unpadded; the same size and sample type go in and out, one output frame per source
 * frame.  For half frames every frame base and frame stride must be even (CRTFX_E_INVALID otherwise); uint8 frames may start anywhere.
 *
 * Stated limits: the rows of a woven interlaced frame are taken as consecutive lines; no 25 Hz offset of the subcarrier; no RF noise.  NTSC
 * has no phase knob: crtfx_signal_* is untouched.  The chroma rows of a 4:2:0 source are formed in front of this stage by its source plan.
 *
 * Paths; both give the same bytes, the path is chosen per run, and *_last_plan names the one that ran.  Thirty-two builds.
 * k_pal<signal,chroma,decoder,pix,vec>: runs where
 *     w % 8 == 0, both frame bases are multiples of 4, and so are both strides where n > 1
 * — the rule of crtfx_signal.h.  One wave takes a segment of 488 pixels (with the halo of 12 to either side that is 512 = 64 lanes x 8) and
 * a strip of 8 consecutive rows of one frame and walks down the strip; four waves a workgroup, all frames of a launch one grid (grid.z;
 * 32768 frames per launch).  For each row the cascade is staged through four int16 planes of the wave's own in LDS exactly as k_signal
 * stages it (crtfx_signal.h), through step 7: whether a sample carries U or V is a constant of its place in the lane's eight that the
 * row's rotation swaps, so the carrier products stay selections and only the one of U1 / V1 that the phase keeps is formed.  Under DELAY
 * the lane keeps the previous row's Ur / Vr of its eight pixels in sixteen registers — the delay line — and first runs the row above the
 * strip (for the strip at row 0: row 1) without storing it: a strip costs 9 cascades for 8 rows.  Under SIMPLE there is no extra row and no
 * carried state.  No wave depends on another wave's result.  Every wave of every workgroup makes the same number of trips and meets two
 * barriers in each: a strip the frame cuts short, and a wave past the last strip, repeat a row and store nothing.
 * k_pal<signal,chroma,decoder,pix,general>: any size and alignment, and the CRTFX_PAL_OPT_FORCE_GENERAL fallback: one lane per pixel
 * evaluates the cascade of that pixel in its row and, under DELAY, in the partner row, from pixels loaded at clamped columns, 1-byte
 * (2-byte) loads and stores; grid = (pixels of a row, rows, frames).
 * Every output element is written by exactly one lane on either path; column and row indices are clamped, not padded, so no byte outside a
 * source frame is read; bytes between frames are neither read nor written.  No inline assembly.
 *
 * Registers (gfx950, as built; tests/test_pal_tables.py reads them from the library): VGPRs of k_pal<signal,chroma,decoder,pix,path>
 *     k_pal<composite,sharp,delay,u8,vec> 85, k_pal<composite,sharp,delay,f16,vec> 85, k_pal<composite,sharp,simple,u8,vec> 70, k_pal<composite,sharp,simple,f16,vec> 68,
 *     k_pal<composite,soft,delay,u8,vec> 105, k_pal<composite,soft,delay,f16,vec> 105, k_pal<composite,soft,simple,u8,vec> 90, k_pal<composite,soft,simple,f16,vec> 93,
 *     k_pal<svideo,sharp,delay,u8,vec> 79, k_pal<svideo,sharp,delay,f16,vec> 77, k_pal<svideo,sharp,simple,u8,vec> 65, k_pal<svideo,sharp,simple,f16,vec> 61,
 *     k_pal<svideo,soft,delay,u8,vec> 103, k_pal<svideo,soft,delay,f16,vec> 101, k_pal<svideo,soft,simple,u8,vec> 85, k_pal<svideo,soft,simple,f16,vec> 88,
 *     k_pal<composite,sharp,delay,u8,general> 121, k_pal<composite,sharp,delay,f16,general> 163, k_pal<composite,sharp,simple,u8,general> 80, k_pal<composite,sharp,simple,f16,general> 92,
 *     k_pal<composite,soft,delay,u8,general> 182, k_pal<composite,soft,delay,f16,general> 232, k_pal<composite,soft,simple,u8,general> 112, k_pal<composite,soft,simple,f16,general> 167,
 *     k_pal<svideo,sharp,delay,u8,general> 96, k_pal<svideo,sharp,delay,f16,general> 112, k_pal<svideo,sharp,simple,u8,general> 61, k_pal<svideo,sharp,simple,f16,general> 67,
 *     k_pal<svideo,soft,delay,u8,general> 171, k_pal<svideo,soft,delay,f16,general> 198, k_pal<svideo,soft,simple,u8,general> 112, k_pal<svideo,soft,simple,f16,general> 117
 * LDS: 16896 bytes per workgroup for every vec build (4 waves x 4 planes x 528 int16), none for the general ones;
 * no AGPRs, no scratch, no spills.
 *
 * Kernel time per frame: measured once on one MI355X in batches of 8 (tools/pal_kernel_times.py, HIP events, launch gaps included;
 * profiles/pal.txt holds the whole output, for strips of 8, 16 and 32 rows), next to the untouched k_signal<same signal,chroma,pix,vec> —
 * the yardstick: the same row cascade without the strip, the rotation and the delay line — and a device-to-device copy of equal traffic
 * (0.41 / 0.66 us at 576 x 720, 1.57 / 2.94 at 1080 x 1920, uint8 / half), all timed in the same run; us, a strip of 8 rows,
 * delay vec / general, simple vec / general, k_signal:
 *                                      uint8                                       half
 *     576 x 720    composite, sharp    4.68 /  20.64, 4.00 /  9.22, 1.68           5.59 /  23.42, 4.95 / 11.05, 2.21
 *                  composite, soft     5.54 /  44.37, 4.83 / 16.64, 1.94           6.48 /  44.17, 5.77 / 19.56, 2.44
 *                  svideo, sharp       4.26 /  14.11, 3.81 /  6.46, 1.52           5.25 /  15.60, 4.65 /  7.68, 2.03
 *                  svideo, soft        5.06 /  35.71, 4.44 / 12.86, 1.69           5.98 /  35.47, 5.31 / 14.13, 2.17
 *     1080 x 1920  composite, sharp    9.01 /  97.59, 7.79 / 44.66, 5.41          10.97 / 114.73, 9.70 / 52.28, 7.01
 *                  composite, soft    11.23 / 223.19, 9.35 / 80.94, 6.41          13.20 / 218.77, 11.20 / 94.79, 8.00
 *                  svideo, sharp       8.26 /  67.78, 7.18 / 30.17, 4.82          10.16 /  74.77, 9.02 / 35.91, 6.31
 *                  svideo, soft       10.06 / 178.98, 8.41 / 63.81, 5.57          11.93 / 174.80, 10.07 / 67.89, 6.99
 * By construction a DELAY strip runs 9 cascades for 8 rows, plus the rotation.  Measured, the vec path takes 1.56 - 1.81 x k_signal under
 * DELAY and 1.38 - 1.51 x under SIMPLE at 1080 x 1920, and 2.53 - 2.99 x / 2.24 - 2.63 x at 576 x 720: well above 9 / 8.  What the strip costs
 * is parallelism — it leaves an eighth of k_signal's waves, each eight or nine cascades long: a batch of 8 frames of 576 x 720 is 1152 waves
 * for the 1024 SIMDs, one wave each with nothing to hide its trips through LDS and its barriers behind, where k_signal has nine.  Taller
 * strips are slower still: 16 rows take 1.95 - 2.18 x k_signal (DELAY, 1080 x 1920) and 3.32 - 4.22 x (576 x 720), 32 rows 2.86 - 3.26 x and
 * 6.26 - 8.06 x, and under 32 rows the general path is the faster one for SIMPLE at 576 x 720 (0.61 - 1.27 x the vec path).  So the strip is
 * 8 rows, the smallest candidate.  With it the general path takes 2.97 - 8.01 x (DELAY) and 1.65 - 3.45 x (SIMPLE) the vec path at 576 x 720
 * and 7.4 - 19.9 x / 4.0 - 8.7 x at 1080 x 1920: vec is the faster path at both sizes for every build, so vec runs whenever its conditions
 * hold.
 */
#ifndef CRTFX_PAL_H
#define CRTFX_PAL_H

#include <stddef.h>
#include <stdint.h>

#include "crtfx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crtfx_pal crtfx_pal;

typedef enum crtfx_pal_kind { CRTFX_PAL_COMPOSITE = 0, CRTFX_PAL_SVIDEO = 1 } crtfx_pal_kind;
typedef enum crtfx_pal_chroma { CRTFX_PAL_SHARP = 0, CRTFX_PAL_SOFT = 1 } crtfx_pal_chroma;
typedef enum crtfx_pal_decoder { CRTFX_PAL_DELAY = 0, CRTFX_PAL_SIMPLE = 1 } crtfx_pal_decoder;

/* Plans the stage for h x w x 3 frames of pix_fmt (CRTFX_PIX_U8 or CRTFX_PIX_F16) on `device` (the calling thread's current device is
 * restored).  crawl is 0 or 1, phase the decoder's phase error in whole degrees.  CRTFX_E_INVALID: a null out pointer, h or w < 1 or
 * > 32767, an unknown pix_fmt, signal, chroma or decoder, a crawl that is neither 0 nor 1, a phase outside -180..180.  All of these are
 * refused before a device is touched.  When it fails *out_plan is NULL and crtfx_pal_last_error(NULL) holds the message (per calling
 * thread), which names the offending field. */
int crtfx_pal_create(int device, int h, int w, int pix_fmt, int signal, int chroma, int crawl, int decoder, int phase, crtfx_pal** out_plan);
int crtfx_pal_destroy(crtfx_pal* plan);
const char* crtfx_pal_last_error(const crtfx_pal* plan);

/* n frames in one call: frame i is read at src_base + i * src_stride_bytes and written at dst_base + i * dst_stride_bytes (h x w x 3
 * samples each, rows unpadded), and its t is first_index + i, of which only t mod 4 matters.  n = 0 does nothing.  The refusals are those
 * of crtfx_signal_run — CRTFX_E_INVALID: a negative first_index, n < 0, a null frame pointer, a stride shorter than a frame (n > 1), an odd
 * base or stride for half frames, and a source range that overlaps the destination's.  Bytes between frames are neither read nor written. */
int crtfx_pal_run(crtfx_pal* plan, int64_t first_index, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes,
                  int n, void* stream);

/* Testing / A-B switches of one plan.  FORCE_GENERAL (0 / 1): take the general kernel whatever the width and alignment. */
typedef enum crtfx_pal_option { CRTFX_PAL_OPT_FORCE_GENERAL = 1 } crtfx_pal_option;
int crtfx_pal_set_option(crtfx_pal* plan, int option, int value);

/* The path of the most recent crtfx_pal_run (before the first one: the path a run with aligned frames takes) and its frames:
 * `pal=k_pal<composite,soft,delay,u8,vec>;frames=5` or `pal=k_pal<svideo,sharp,simple,f16,general>;frames=1`. */
int crtfx_pal_last_plan(crtfx_pal* plan, char* buf, size_t n);

/* Step 7's table, without a device: *c = llrint(4096 cos theta), *s = llrint(4096 sin theta) for theta = degrees, in double.
 * CRTFX_E_INVALID: degrees outside -180..180 or a null pointer. */
int crtfx_pal_phase_table(int degrees, int* c, int* s);

#ifdef __cplusplus
}
#endif
#endif /* CRTFX_PAL_H */
