/*
 * crtfx_egress_sited.h — the sited egress stage of libcrtfx.so: finished RGB frames converted to the seven sub-sampled layouts the other
 * egress stages write (crtfx_egress_*, crtfx_egress422_*, crtfx_egress10_*) with the chroma samples FILTERED onto a stated siting instead of
 * taken as the 2 x 2 / 2 x 1 box mean.  The box mean is centre siting; a yuv420p file muxed by ffmpeg is tagged or assumed
 * chroma_location=left, and 4:2:2 formats define no other siting, so box chroma sits a quarter luma pixel to the right of where every
 * player and re-encoder places it.  The stage stands where the box one stood: same RGB frames in, same frames out, the same seven entry
 * points (crtfx_egress.h), one more option.  It is the mirror image of the sited source stage (crtfx_sited.h) and reuses its layout and
 * siting enumerations.
 *
 * Status codes (crtfx_status), pixel formats (crtfx_pixfmt) and conventions are those of crtfx.h: the caller owns every frame; work is
 * enqueued on the caller's hipStream_t (void*, NULL = the default stream); only create / destroy synchronise; the calling thread's current
 * device must be the plan's when it runs.
 *
 * Layouts (crtfx_sited_layout), with cw = (w + 1) / 2 and ch = (h + 1) / 2, every row unpadded:
 *     yuv420p, nv12                 the geometry of crtfx_egress.h      frame_bytes = h * w + 2 * ch * cw             uint8 h x w x 3 in
 *     yuv422p, yuyv422, uyvy422     the geometry of crtfx_422.h         h * w + 2 * h * cw (planar), 4 * h * cw       uint8 h x w x 3 in
 *                                   (the pad byte of an odd-width packed row is a copy of the row's last Y)
 *     yuv420p10le, p010le           the geometry of crtfx_deep.h        2 * (h * w + 2 * ch * cw)                     half h x w x 3 in
 *                                   word = v / v << 6, the bits outside a sample written 0
 * The RGB pixel format follows from the layout: CRTFX_PIX_U8 for the five 8-bit layouts, CRTFX_PIX_F16 (0..255 scale) for the two 10-bit ones.
 *
 * Arithmetic.  Exact integers, one shift, one clamp.  The per-pixel code p is the uint8 channel value (8-bit) or the quarter code
 * q = rint_to_even(min(max(4 f, 0), 1020)), NaN -> 0, of the half f (10-bit: exactly crtfx_deep.h's quantiser).  Y is the box stage's Y,
 * unchanged: Y[y][x] = clamp((m0 . p[y][x] + (off0 << 16) + (1 << 15)) >> 16, 0, T), T = 255 (8-bit) or 1023 (10-bit).  m = rows Y, U, V of a
 * 3 x 3 integer matrix over the columns (R, G, B), off1 and off2 are 128 or 512.  For chroma sample (cy, cx), per channel:
 *     x0 = 2 cx, xl = max(x0 - 1, 0), xr = min(x0 + 1, w - 1)
 *     H[y][cx]  = wl * p[y][xl] + w0 * p[y][x0] + wr * p[y][xr]
 *                 (wl, w0, wr) = (1, 2, 1) left, (0, 2, 2) center                                  weights in quarters, sum 4
 *     4:2:0:  S = H[y0][cx] + H[y1][cx],  y0 = 2 cy, y1 = min(y0 + 1, h - 1)
 *             U = clamp((m1 . S + (off1 << 19) + (1 << 18)) >> 19, 0, T)                           V likewise with m2, off2
 *     4:2:2:  S = H[y][cx]
 *             U = clamp((m1 . S + (off1 << 18) + (1 << 17)) >> 18, 0, T)                           V likewise with m2, off2
 * "left": the sample sits on luma column 2 cx (MPEG-2 / H.264 / HEVC; the only siting 4:2:2 defines); horizontally the filter is
 * [1 2 1] / 4 centred there.  Vertically a 4:2:0 sample sits midway between its two rows at both sitings, as in crtfx_sited.h.  Edge taps
 * are clamped indices: nothing outside the frame is read.  "center": S is exactly twice the box stages' sum and the shift has one more
 * bit — 2 A + 2 B >> (n + 1) = A + B >> n for every integer, rounding term included — so the bytes are those of crtfx_egress_* /
 * crtfx_egress422_* / crtfx_egress10_* for EVERY input: the counterpart of the source stage's "equal taps" identity.  m and off are those
 * stages' (pythoncrt_amd.tables.yuv_matrix, yuv_matrix10).  NOT claimed: byte equality with libswscale.  What the tests hold the kernels
 * to is the arithmetic above (tests/egress_sited_model.py).
 *
 * The matrices create admits (CRTFX_E_INVALID otherwise).  Per row, with K the constant term and P / N the sums of the row's positive /
 * negative entries: K + N * X >= 0 and K + P * X < 2^31, so every accumulator stays in [0, 2^31) for every input, the lower clamp never acts
 * and the kernels shift unsigned.  Y row: K = (off0 << 16) + (1 << 15), X = 255 or 1020 (the box stages' rule).  Chroma rows: K as above,
 * X = 8 * 255 (8-bit 4:2:0), 4 * 255 (4:2:2), 8 * 1020 (10-bit).  All eight shipped matrices pass; their largest chroma accumulator is
 * 0.0625 * 2^31 (8-bit) and 0.25 * 2^31 (10-bit).
 *
 * Paths, chosen per run and named by crtfx_egress_sited_last_plan; both give the same bytes.  Fourteen kernels, k_egress_sited<layout, path>;
 * the siting travels as the three weights in the kernel arguments, so one build serves both sitings.
 *     vec       taken when w % 8 == 0 and the frame bases are 4-byte aligned: src_base and dst_base are multiples of 4, and with n > 1 so
 *               are both strides (the other stages' rule).  One lane owns 8 columns of two rows (4:2:0) or one row (4:2:2): its RGB, its
 *               Y and its four chroma samples per plane are the dword-multiple accesses of the box stage's vec kernel of that layout.
 *               Consecutive lanes take consecutive column blocks; all n frames are one grid.  xr always lies inside the lane's block; the
 *               only sample outside it is the pixel left of the block (x = 8 * block - 1, clamped to 0 at the row start), used by the lane's
 *               first chroma sample.  It is read with ONE NARROW LOAD per row at the clamped index (3 bytes, or 3 halves through the
 *               quantiser), the source stage's form: a wave end and a row start need no special case.  The alternative — the neighbour
 *               lane's last pixel through a cross-lane move — was not built.  An odd h is served: the last lane row stores one Y row and
 *               uses y1 = y0.
 *     general   any size and alignment (10-bit: even bases and strides): one lane per chroma sample and the up to 2 x 2 (4:2:0) or 2 x 1
 *               (4:2:2) Y samples under it, byte loads and stores (10-bit: 16-bit ones).  Every output element, the pad byte of a packed
 *               row included, is written by exactly one lane and nothing beyond x < w, y < h is read.  Also the A/B and test fallback
 *               (CRTFX_EGRESS_SITED_OPT_FORCE_GENERAL).
 * Registers (gfx950, as built; tests/test_egress_sited_tables.py reads them from the library and holds every build to 128): VGPRs of
 * <layout>: vec / general —
 *     yuv420p 70 / 30     nv12 70 / 30     yuv422p 38 / 17     yuyv422 35 / 17     uyvy422 35 / 17     yuv420p10le 77 / 28     p010le 77 / 27
 * The 4:2:0 vec builds hold two rows of eight RGB pixels (2 x 6 dwords, 10-bit: 2 x 12) beside the left pixel of each row and pass 64: seven
 * waves per SIMD instead of eight, as the 10-bit box kernel (71);
 * no AGPRs, no LDS, no scratch, no spills.
 * Measured once on one MI355X, batches of 8 frames (profiles/egress_sited.txt, tools/egress_sited_kernel_times.py): at 4K the vec builds take
 * 6.7 us per frame (yuv420p, nv12), 8.2 - 8.3 us (the 4:2:2 layouts) and 13.8 - 14.1 us (10-bit) at siting left, 1.03 - 1.13 x the box stages' vec
 * builds of the same run and 0.97 - 1.08 x a device-to-device copy of the same traffic, and every vec build is 1.40 - 2.54 x faster than its
 * general build (1.30 - 2.15 x at 1080p): "vec whenever its conditions hold" stands for all seven layouts.  The two sitings differ by at most
 * 0.2 us, as run-time weights should.  The narrow-load form above is the one that was built and measured; the cross-lane form was not.
 */
#ifndef CRTFX_EGRESS_SITED_H
#define CRTFX_EGRESS_SITED_H

#include <stddef.h>
#include <stdint.h>

#include "crtfx.h"
#include "crtfx_sited.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crtfx_egress_sited crtfx_egress_sited;

/* Plans the conversion on `device` (synchronises; the calling thread's current device is restored).  layout is a crtfx_sited_layout.
 * pix_fmt, the format of the RGB frames read, must be the one the layout implies; the other one is CRTFX_E_UNSUPPORTED.  m: 9 integers
 * (rows Y, U, V over the columns R, G, B), off: 3 integers in 0..255 (8-bit layouts) or 0..1023 (10-bit).  CRTFX_E_INVALID: a size < 1 or
 * > 32767, an unknown layout or pixel format, a null table, an offset outside its range, or a matrix the rules above do not admit.  All of
 * these are refused before a device is touched.  When it fails *out_plan is NULL and crtfx_egress_sited_last_error(NULL) holds the
 * message (per calling thread).  The siting of a new plan is CRTFX_SITED_LEFT. */
int crtfx_egress_sited_create(int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, crtfx_egress_sited** out_plan);
int crtfx_egress_sited_destroy(crtfx_egress_sited* plan);
const char* crtfx_egress_sited_last_error(const crtfx_egress_sited* plan);

/* The bytes of one frame WRITTEN (the layout's expression above); 0 for a null plan. */
size_t crtfx_egress_sited_frame_bytes(const crtfx_egress_sited* plan);

/* n frames in one call: frame i is read at src_base + i * src_stride_bytes (h x w x 3 bytes or halves, rows unpadded) and written at
 * dst_base + i * dst_stride_bytes (frame_bytes bytes); strides of at least a frame.  The 8-bit layouts take any byte base and stride; the
 * 10-bit ones need even bases and strides (CRTFX_E_INVALID otherwise).  Bytes between frames are neither read nor written.  Source and
 * destination must not overlap. */
int crtfx_egress_sited_run(crtfx_egress_sited* plan, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream);

/* FORCE_GENERAL (0 / 1): take the narrow-access kernel whatever the width and alignment.  SITING (CRTFX_SITED_LEFT / CRTFX_SITED_CENTER):
 * the horizontal siting of the runs that follow; a live plan may be switched back and forth.  Any other option or value: CRTFX_E_INVALID. */
typedef enum crtfx_egress_sited_option { CRTFX_EGRESS_SITED_OPT_FORCE_GENERAL = 1, CRTFX_EGRESS_SITED_OPT_SITING = 2 } crtfx_egress_sited_option;
int crtfx_egress_sited_set_option(crtfx_egress_sited* plan, int option, int value);

/* The path of the most recent crtfx_egress_sited_run (before the first one: the path a run with aligned bases would take) and the siting:
 * `egress_sited=k_egress_sited<nv12,vec>;siting=left;frames=5` or `egress_sited=k_egress_sited<p010le,general>;siting=center;frames=5`. */
int crtfx_egress_sited_last_plan(crtfx_egress_sited* plan, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* CRTFX_EGRESS_SITED_H */
