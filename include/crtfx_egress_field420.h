/*
 * crtfx_egress_field420.h — the field-paired 4:2:0 egress stage of libcrtfx.so: finished RGB frames converted to the four 4:2:0 layouts the
 * other egress stages write (crtfx_egress_*, crtfx_egress10_*, crtfx_egress_sited_*) with every chroma sample formed from luma rows of ITS
 * OWN FIELD only.  An interlaced decoder (MPEG-2, H.264 and HEVC at 480i / 576i / 1080i, and crtfx_field420_* here) reads chroma rows
 * 0, 2, 4, ... as the top field's (luma rows 0, 2, 4, ...) and chroma rows 1, 3, 5, ... as the bottom field's.  The progressive stages form
 * chroma row c from luma rows 2c and 2c + 1, one row of each field, so a woven frame (crtfx_interlace.h) leaves them with the colour of two
 * moments 1/60 s apart mixed in every chroma sample: coloured combing on motion.  The stage stands where the box and the sited one stand:
 * same RGB frames in, same frames out, the same seven entry points (crtfx_egress.h), one more option.  It is the mirror image of the
 * field-paired source stage (crtfx_field420.h) and reuses its layout enumeration.
 *
 * Status codes (crtfx_status), pixel formats (crtfx_pixfmt) and conventions are those of crtfx.h: the caller owns every frame; work is
 * enqueued on the caller's hipStream_t (void*, NULL = the default stream); only create / destroy synchronise; the calling thread's current
 * device must be the plan's when it runs.
 *
 * Geometry.  h is a multiple of 4 and at least 4, w is any size from 1 to 32767; cw = (w + 1) / 2, ch = h / 2, every row unpadded:
 *     yuv420p, nv12                 the layouts of crtfx_egress.h       frame_bytes = h * w + 2 * ch * cw             uint8 h x w x 3 in
 *     yuv420p10le, p010le           the layouts of crtfx_deep.h         2 * (h * w + 2 * ch * cw)                     half h x w x 3 in
 *                                   word = v / v << 6, the bits outside a sample written 0
 * The RGB pixel format follows from the layout: CRTFX_PIX_U8 for the two 8-bit layouts, CRTFX_PIX_F16 (0..255 scale) for the two 10-bit
 * ones.  h % 4 == 2 is deliberately NOT served: the bottom field's last luma row would then lie under no chroma row of its own (the field
 * has an odd number of rows, ch / 2 rounds down for it), and whatever row it were folded into would carry the sample off its siting.  The
 * interlaced rasters in use (480, 576, 1080 rows) are all multiples of 4.
 *
 * Arithmetic.  Exact integers, one shift, one clamp, in the style of crtfx_egress_sited.h.  The per-pixel code p is the uint8 channel value
 * (8-bit) or the quarter code q = rint_to_even(min(max(4 f, 0), 1020)), NaN -> 0, of the half f (10-bit: exactly crtfx_deep.h's
 * quantiser).  Y is the box stages' Y, unchanged, for every pixel: Y[y][x] = clamp((m0 . p[y][x] + (off0 << 16) + (1 << 15)) >> 16, 0, T),
 * T = 255 or 1023.  m = rows Y, U, V of a 3 x 3 integer matrix over the columns (R, G, B), off1 and off2 are 128 or 512.  Chroma row c
 * belongs to field f = c & 1 and is that field's chroma row i = c >> 1; field f's luma rows are frame rows 2 k + f, k = 0 .. ch - 1.  For
 * chroma sample (c, cx), per channel:
 *     x0 = 2 cx, xl = max(x0 - 1, 0), xr = min(x0 + 1, w - 1)
 *     H[y][cx]  = wl * p[y][xl] + w0 * p[y][x0] + wr * p[y][xr]
 *                 (wl, w0, wr) = (1, 2, 1) left, (0, 2, 2) center                    crtfx_egress_sited.h's taps; weights in quarters, sum 4
 *     S[c][cx]  = sum over t = 0..3 of v_t * H[2 * clamp(2 i - 1 + t, 0, ch - 1) + f][cx]
 *                 (v_0 .. v_3), in sixteenths:   center  (0, 8, 8, 0) for both fields
 *                                                left    (3, 7, 5, 1) top field,  (1, 5, 7, 3) bottom field
 *     U = clamp((m1 . S + (off1 << 22) + (1 << 21)) >> 22, 0, T)                     V likewise with m2, off2; weights sum to 4 * 16 = 64
 * "left" is MPEG-2's interlaced siting (v_chr_pos 64 / 192 in ffmpeg's terms): a top-field sample sits a quarter field row below field row
 * 2 i, a bottom-field one three quarters below, and horizontally both sit on luma column 2 cx.  The four vertical weights are the triangle
 * of half-width two field rows centred there — the vertical counterpart of the horizontal [1 2 1] / 4 — and the transpose of the (7, 1) /
 * (5, 3) eighths by which crtfx_field420.h interpolates.  "center" is the box mean inside the field.  Edge taps are clamped indices:
 * nothing outside the frame is read.  m and off are the other egress stages' (pythoncrt_amd.tables.yuv_matrix, yuv_matrix10).  NOT
 * claimed: byte equality with libswscale.  What the tests hold the kernels to is the arithmetic above (tests/egress_field420_model.py).
 *
 * Consequences.
 *     Under "center" the frame is the weave of crtfx_egress_* / crtfx_egress10_* run on each field as an h/2 x w frame of its own (field f:
 *     luma rows f, f + 2, ..., chroma rows f, f + 2, ...), for EVERY input: S is 16 times those stages' box sum A and the shift has four
 *     more bits, and (16 A m + (off << 22) + (1 << 21)) >> 22 = (A m + (off << 18) + (1 << 17)) >> 18 for every integer.
 *     A frame whose two fields are each a flat colour gives, on the chroma rows of field f, the box stages' bytes for a flat frame of that
 *     field's colour, under both chroma values: every tap of a sample reads its own field, so S = 64 p.
 *     A field holding a vertical linear ramp (p = a + b k on field row k, constant in x) gives S / 64 equal to the ramp's value at the
 *     sample's siting — a + b (2 i + 1/4) top, a + b (2 i + 3/4) bottom under "left", a + b (2 i + 1/2) under "center" — exactly, on every
 *     chroma row whose four taps are unclamped.
 *     A change confined to one field's rows changes no chroma sample of the other field.
 *
 * Accumulator width and the matrices create admits (CRTFX_E_INVALID otherwise).  Per row, with K the constant term and P / N the sums of
 * the row's positive / negative entries, every code lies in [0, X], so the integer accumulator A lies in [K + N * X, K + P * X].
 *     Y rows      K = (off0 << 16) + (1 << 15), X = 255 or 1020:  K + N * X >= 0 and K + P * X < 2^31, the box stages' rule.
 *     8-bit chroma  K = (off << 22) + (1 << 21), X = 64 * 255:    K + N * X >= 0 and K + P * X < 2^31.  The four shipped matrices stay at or
 *                 below 0.5 * 2^31.
 *     10-bit chroma X = 64 * 1020:  the shipped matrices reach 1.876 * 2^31 (limited range) and 1.99999 * 2^31 (full range), so int32 does
 *                 not hold them.  The rule is K + N * X >= 0 and K + P * X < 2^32, and the kernels accumulate in UNSIGNED 32-bit words.
 *                 Proof: unsigned arithmetic is arithmetic modulo 2^32, and a negative entry enters as its two's complement, which is
 *                 congruent to it; so the word the kernel holds after the three products and the constant is congruent to A modulo 2^32,
 *                 whatever the intermediate sums did.  Under the rule 0 <= A < 2^32, and the word lies there too: they are equal.  The
 *                 logical shift is then floor(A / 2^22), the lower clamp never acts and the upper one is an unsigned minimum: the
 *                 int64 model's code, for every input and every admitted matrix.  The eight shipped matrices keep K + N * X at or above
 *                 0.0019 * 2^31.  No 64-bit accumulation anywhere.
 *     The same unsigned form serves the 8-bit builds and every Y, whose narrower rules it covers.
 *
 * Paths, chosen per run and named by crtfx_egress_field420_last_plan; both give the same bytes.  Eight kernels,
 * k_egress_field420<layout, path>; the chroma option travels as the three horizontal and twice four vertical weights in the kernel
 * arguments, so one build serves both values.
 *     vec       taken when w % 8 == 0 and the frame bases are 4-byte aligned: src_base and dst_base are multiples of 4, and with n > 1 so
 *               are both strides (the other stages' rule).  One lane owns 8 columns of the two luma rows that share a field chroma row,
 *               frame rows 4 i + f and 4 i + 2 + f: their Y and its four chroma samples per plane are the dword-multiple stores of
 *               k_egress_sited's vec build of that layout.  It additionally reads the field row above and the one below, at clamped
 *               indices, for the two outer taps: four dword-multiple row loads, one row in hand at a time, each row's H added into twelve
 *               running weighted sums.  The pixel left of the block comes from one narrow load per row at a clamped index, as in
 *               k_egress_sited.  Lane rows alternate between the fields, so consecutive lane rows touch consecutive frame rows.
 *     general   any size and alignment (10-bit: even bases and strides): one lane per chroma sample and the up to 2 x 2 Y samples of its
 *               field under it, byte loads and stores (10-bit: 16-bit ones); 4 x 3 taps at clamped indices.  Every output element is
 *               written by exactly one lane and nothing beyond x < w is read or written at an odd width.  Also the A/B and test fallback
 *               (CRTFX_EGRESS_FIELD420_OPT_FORCE_GENERAL).
 * Registers (gfx950, as built; tests/test_egress_field420_tables.py reads them from the library and holds every build to 128): VGPRs of
 * <layout>: vec / general —
 *     yuv420p 48 / 50     nv12 46 / 50     yuv420p10le 64 / 47     p010le 102 / 47
 * no AGPRs, no LDS, no scratch, no spills.
 * Measured once on one MI355X, batches of 8 frames (profiles/egress_field420.txt, tools/egress_field420_kernel_times.py), beside the untouched
 * k_egress_sited<layout,vec> at siting left — the same bytes out, one RGB read where this stage has up to two — and a device-to-device copy
 * of equal traffic in the same run.  The vec builds take 9.1 - 9.2 us per frame at 4K for the 8-bit layouts and 18.0 - 19.4 us for the 10-bit
 * ones: 1.38 - 1.42 x and 1.30 - 1.38 x the sited vec build (6.4 - 6.7 / 13.8 - 14.1 us), 1.31 - 1.41 x the copy.  At 1080 x 1920: 2.5 - 2.6 us
 * and 4.6 us, 1.38 - 1.39 x and 1.50 - 1.51 x the sited build, 1.71 - 1.80 x the copy (the batches are cache-resident there, so the copy is a
 * hard yardstick).  The extra over the sited build is the two outer taps: four row loads and four rows of H where that build has two.  The
 * two chroma values differ by at most 0.07 us at 4K and 0.01 us at 1080 x 1920, as run-time weights should.  Every vec build is 1.39 - 2.52 x
 * faster than its general build at 1080 x 1920 and 1.67 - 2.79 x at 4K.  At 480 x 720 in batches of 8 every row of the table, the sited
 * kernels included, is a launch-bound 1.33 - 1.41 us per frame, vec and general within 5 % of each other either way round; the same size in
 * batches of 64, where the kernels are the bound, has vec at 0.40 - 0.72 us and general at 1.04 - 1.07 us, 1.48 - 2.58 x.  The general path is
 * measurably faster nowhere, so "vec whenever its conditions hold" stands.
 */
#ifndef CRTFX_EGRESS_FIELD420_H
#define CRTFX_EGRESS_FIELD420_H

#include <stddef.h>
#include <stdint.h>

#include "crtfx.h"
#include "crtfx_field420.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crtfx_egress_field420 crtfx_egress_field420;

typedef enum crtfx_egress_field420_chroma { CRTFX_EGRESS_FIELD420_CENTER = 0, CRTFX_EGRESS_FIELD420_LEFT = 1 } crtfx_egress_field420_chroma;

/* Plans the conversion on `device` (synchronises; the calling thread's current device is restored).  layout is a crtfx_field420_layout.
 * pix_fmt, the format of the RGB frames read, must be the one the layout implies; the other one is CRTFX_E_UNSUPPORTED.  m: 9 integers
 * (rows Y, U, V over the columns R, G, B), off: 3 integers in 0..255 (8-bit layouts) or 0..1023 (10-bit).  CRTFX_E_INVALID: an h that is
 * no multiple of 4 or below 4, a size > 32767 or a w < 1, an unknown layout or pixel format, a null table, an offset outside its range, or
 * a matrix the rules above do not admit.  All of these are refused before a device is touched.  When it fails *out_plan is NULL and
 * crtfx_egress_field420_last_error(NULL) holds the message (per calling thread).  The chroma of a new plan is CRTFX_EGRESS_FIELD420_CENTER. */
int crtfx_egress_field420_create(int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, crtfx_egress_field420** out_plan);
int crtfx_egress_field420_destroy(crtfx_egress_field420* plan);
const char* crtfx_egress_field420_last_error(const crtfx_egress_field420* plan);

/* The bytes of one frame WRITTEN (the layout's expression above); 0 for a null plan. */
size_t crtfx_egress_field420_frame_bytes(const crtfx_egress_field420* plan);

/* n frames in one call: frame i is read at src_base + i * src_stride_bytes (h x w x 3 bytes or halves, rows unpadded) and written at
 * dst_base + i * dst_stride_bytes (frame_bytes bytes); strides of at least a frame.  The 8-bit layouts take any byte base and stride; the
 * 10-bit ones need even bases and strides (CRTFX_E_INVALID otherwise).  Bytes between frames are neither read nor written.  Source and
 * destination must not overlap. */
int crtfx_egress_field420_run(crtfx_egress_field420* plan, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream);

/* FORCE_GENERAL (0 / 1): take the narrow-access kernel whatever the width and alignment.  CHROMA (CRTFX_EGRESS_FIELD420_CENTER / _LEFT):
 * where the chroma samples of the runs that follow sit inside their field; a live plan may be switched back and forth.  Any other option
 * or value: CRTFX_E_INVALID. */
typedef enum crtfx_egress_field420_option { CRTFX_EGRESS_FIELD420_OPT_FORCE_GENERAL = 1, CRTFX_EGRESS_FIELD420_OPT_CHROMA = 2 } crtfx_egress_field420_option;
int crtfx_egress_field420_set_option(crtfx_egress_field420* plan, int option, int value);

/* The path of the most recent crtfx_egress_field420_run (before the first one: the path a run with aligned bases would take) and the
 * chroma: `egress_field420=k_egress_field420<nv12,vec>;chroma=left;frames=5` or
 * `egress_field420=k_egress_field420<p010le,general>;chroma=center;frames=5`. */
int crtfx_egress_field420_last_plan(crtfx_egress_field420* plan, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* CRTFX_EGRESS_FIELD420_H */
