/*
 * crtfx_field420.h — the field-paired 4:2:0 source stage of libcrtfx.so: the four 4:2:0 layouts the other source stages read (crtfx_unpack_*,
 * crtfx_unpack10_*, crtfx_sited_*) converted to RGB with every luma row taking its chroma from rows of ITS OWN FIELD only.  An interlaced
 * encoder (MPEG-2, H.264 and HEVC at 480i / 576i / 1080i) sub-samples each field on its own: chroma rows 0, 2, 4, ... belong to the top field
 * (luma rows 0, 2, 4, ...) and chroma rows 1, 3, 5, ... to the bottom field.  The progressive stages spread chroma row c over luma rows 2c and
 * 2c + 1, one row of each field, so frame rows 4j + 1 and 4j + 2 take the other field's colour: coloured combing on motion that no
 * deinterlacer behind the stage can remove.  The stage stands where the replicating and the sited one stand: same frames in, same RGB frames
 * out, the same seven entry points (crtfx_unpack.h), one more option.
 *
 * Status codes (crtfx_status), pixel formats (crtfx_pixfmt) and conventions are those of crtfx.h: the caller owns every frame; work is
 * enqueued on the caller's hipStream_t (void*, NULL = the default stream); only create / destroy synchronise; the calling thread's current
 * device must be the plan's when it runs.
 *
 * Geometry.  h is even and at least 4, w is any size >= 1; cw = (w + 1) / 2, ch = h / 2, every row unpadded:
 *     yuv420p, nv12                 the layouts of crtfx_unpack.h       frame_bytes = h * w + 2 * ch * cw             uint8 h x w x 3 out
 *     yuv420p10le, p010le           the layouts of crtfx_deep.h         2 * (h * w + 2 * ch * cw)                     half h x w x 3 out
 *                                   sample = word & 1023 / word >> 6, the other bits ignored; quarter codes q, out = half(q / 4)
 * The RGB pixel format follows from the layout: CRTFX_PIX_U8 for the two 8-bit layouts, CRTFX_PIX_F16 for the two 10-bit ones.
 *
 * Arithmetic.  Exact integers, one shift, one clamp.  C is a chroma plane of ch x cw samples.
 *     vertical      luma row y has field f = y & 1, field row k = y >> 1 and field chroma row j = k >> 1.  Field f owns
 *                   n_f = (ch + 1 - f) / 2 chroma rows; its chroma row i is frame chroma row 2 i + f.  A top-field chroma row sits a quarter
 *                   field row below its first luma row, a bottom-field one three quarters below (MPEG-2 interlaced siting; v_chr_pos 64 /
 *                   192 in ffmpeg's terms).  With chroma LEFT or CENTER the weights, in eighths:
 *                       top field,    k even   (vn, vf) = (7, 1), far row j - 1          top field,    k odd   (5, 3), far row j + 1
 *                       bottom field, k even   (vn, vf) = (5, 3), far row j - 1          bottom field, k odd   (7, 1), far row j + 1
 *                   Both field chroma rows, near and far, are clamped to [0, n_f - 1]: with h % 4 == 2 the bottom field's last luma row
 *                   reads its last own chroma row.  cy = 2 clamp(j) + f, cyf = 2 clamp(j -+ 1) + f.
 *                   With chroma REPLICATE (vn, vf) = (8, 0): the nearest chroma row of the same field.
 *     horizontal    the (cx, cxf, hn, hf) of crtfx_sited.h, in quarters, for LEFT and CENTER; (hn, hf) = (4, 0) for REPLICATE.
 *     D(C)   = vn * (hn * C[cy][cx] + hf * C[cy][cxf]) + vf * (hn * C[cyf][cx] + hf * C[cyf][cxf])                 weights sum to 32
 *     acc[k] = 32 * m[k][0] * (Y[y][x] - off0) + m[k][1] * (D(U) - 32 * off1) + m[k][2] * (D(V) - 32 * off2) + (1 << 20)      k = R, G, B
 *     8-bit:   out[k] = clamp(acc[k] >> 21, 0, 255)
 *     10-bit:  q[k] = clamp(acc[k] >> 21, 0, 1020),  out[k] = half(q[k] / 4)                                         exact: no rounding occurs
 * Edge taps are clamped indices: nothing outside the planes is read.  m and off are the other source stages' (pythoncrt_amd.tables.rgb_matrix,
 * rgb_matrix10).  NOT claimed: byte equality with libswscale.  What the tests hold the kernels to is the arithmetic above
 * (tests/field420_model.py).
 *
 * Consequences.
 *     Where the taps of a pixel are equal the result is the replicating stage's: acc = 32 * A + 2^20 with A that stage's accumulator
 *     without its rounding term, and floor((32 A + 2^20) / 2^21) = floor((A + 2^15) / 2^16).  So a frame with constant chroma planes converts
 *     to the bytes of crtfx_unpack_* / crtfx_unpack10_* under all three chroma values.
 *     With REPLICATE and h % 4 == 0 the frame is the weave of crtfx_unpack_* / crtfx_unpack10_* run on each field as an h/2 x w frame of its
 *     own (field f: luma rows f, f + 2, ..., chroma rows f, f + 2, ...).
 *
 * Accumulator width and the matrices create admits (every row k; CRTFX_E_INVALID otherwise):
 *     8-bit    (|m[k][0]| + |m[k][1]| + |m[k][2]|) * 255 * 32 + 2^20 < 2^31: acc stays in int32 for every input and every offset.  The four
 *              matrices of tables.rgb_matrix pass; the largest sum is bt709 limited range, about 1.75e9.
 *     10-bit   does not fit int32, neither whole nor split into a luma and a chroma part as crtfx_sited.h splits it: the limited-range luma
 *              part alone reaches 2.34e9 and the chroma part 2.17 - 2.27e9.  The kernels rearrange it.  With c = Y - off0,
 *              d = D(U) - 32 * off1 = 32 * dq + dr and e = D(V) - 32 * off2 = 32 * eq + er (dq = floor(d / 32), 0 <= dr < 32, likewise e):
 *                  acc = 32 * S + R,   S = m0 * c + m1 * dq + m2 * eq,   R = m1 * dr + m2 * er + 2^20
 *                  floor(acc / 2^21) = floor((S + floor(R / 32)) / 2^16)
 *              because S is an integer (floor((32 S + R) / 32) = S + floor(R / 32)) and floor(floor(x / 32) / 2^16) = floor(x / 2^21).
 *              |c|, |dq|, |eq| <= 1023 and |floor(R / 32)| <= |m1| + |m2| + 2^15, so with (|m0| + |m1| + |m2|) * 1024 + 2^15 < 2^31 — the
 *              admission rule — S, R and their sum stay in int32 for every input and every offset, and the code is the int64 model's
 *              for every admitted matrix.  The eight matrices of tables pass by a factor of more than 6.
 *     Either rule holds every entry below 2^22 in magnitude, and every other factor (a weight, a sample, a blend, c, d, e) below 2^16:
 *     the kernels multiply with the 24-bit form (__mul24), whose product of such factors is the exact one.
 *
 * Paths, chosen per run and named by crtfx_field420_last_plan; both give the same bytes.  Eight kernels, k_unpack_field420<layout, path>; the
 * chroma option travels as the horizontal and vertical weights in the kernel arguments.
 *     vec       taken when w % 8 == 0 and the frame bases are 4-byte aligned: src_base and dst_base are multiples of 4, and with n > 1 so
 *               are both strides (the other stages' rule).  One lane owns 8 columns of the two luma rows of one field that share a field
 *               chroma row, frame rows 4 j + f and 4 j + 2 + f (with h % 4 == 2 the last lane row of either field stores one row): its luma,
 *               its four chroma samples per plane and chroma row, and its RGB are dword-multiple accesses.  It reads three chroma rows of
 *               its field: above, own, below, clamped at the field's edges — the register picture of the sited vec builds with doubled
 *               row strides.  The chroma sample to the left and to the right of the lane's four is read with one narrow load each per
 *               chroma row and plane at a clamped index, as in the sited stage.  Lane rows alternate between the fields, so consecutive
 *               lane rows read consecutive frame rows.
 *     general   any size and alignment (10-bit: even bases and strides): one lane per chroma sample position of a field and the up to
 *               2 x 2 pixels of that field under it, byte loads and stores (10-bit: 16-bit ones); 3 x 3 chroma taps per plane at clamped
 *               indices.  Every output element is written by exactly one lane and nothing beyond x < w is read or written at an odd
 *               width.  Also the A/B and test fallback (CRTFX_FIELD420_OPT_FORCE_GENERAL).
 * Registers (gfx950, as built; tests/test_field420_tables.py reads them from the library and holds every build to 128): VGPRs of
 * <layout>: vec / general —
 *     yuv420p 67 / 39     nv12 61 / 28     yuv420p10le 65 / 37     p010le 62 / 31
 * no AGPRs, no LDS, no scratch, no spills.
 * Measured once on one MI355X, batches of 8 frames (profiles/field420.txt, tools/field420_kernel_times.py), beside the untouched
 * k_unpack_sited<layout,vec> at siting left — the same bytes, the same tap count — and a device-to-device copy of equal traffic in the same
 * run.  The vec builds take 11.2 - 11.6 us per frame at 4K for the 8-bit layouts and 21.5 - 23.1 us for the 10-bit ones: 1.04 - 1.10 x and
 * 1.01 x the sited vec build, 1.59 - 1.76 x the copy.  At 1080 x 1920: 3.08 - 3.11 us and 4.45 - 4.57 us, 1.08 - 1.15 x the sited build (the
 * batches are cache-resident there, so the copy is a hard yardstick: 1.67 - 2.24 x).  "replicate" and "left" differ by at most 0.02 us, as
 * run-time weights should.  The extra over the sited build is arithmetic, not the doubled chroma row stride: run-time vertical weights
 * (two multiplies where that build shifts and adds for its fixed 3 : 1) and, for 10 bits, the two sums of the rearrangement; a first build
 * that accumulated the 10-bit layouts in 64 bits took 5.3 - 5.5 us at 1080 x 1920 (1.32 - 1.34 x) and was replaced.  Every vec build is
 * 1.06 - 1.47 x faster than its general build at 1080 x 1920 and at 4K.  At 480 x 720 every row of the table, both yardstick kernels
 * included, is the same launch-bound 1.25 - 1.28 us per frame: there neither path is measurably faster, so "vec whenever its conditions
 * hold" stands.
 */
#ifndef CRTFX_FIELD420_H
#define CRTFX_FIELD420_H

#include <stddef.h>
#include <stdint.h>

#include "crtfx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crtfx_field420 crtfx_field420;

typedef enum crtfx_field420_layout {
    CRTFX_FIELD420_YUV420P = 0, CRTFX_FIELD420_NV12 = 1, CRTFX_FIELD420_YUV420P10LE = 2, CRTFX_FIELD420_P010LE = 3
} crtfx_field420_layout;

typedef enum crtfx_field420_chroma { CRTFX_FIELD420_REPLICATE = 0, CRTFX_FIELD420_LEFT = 1, CRTFX_FIELD420_CENTER = 2 } crtfx_field420_chroma;

/* Plans the conversion on `device` (synchronises; the calling thread's current device is restored).  pix_fmt, the format of the RGB frames
 * written, must be the one the layout implies; the other one is CRTFX_E_UNSUPPORTED.  m: 9 integers (rows R, G, B over the columns Y, U, V),
 * off: 3 integers in 0..255 (8-bit layouts) or 0..1023 (10-bit).  CRTFX_E_INVALID: an odd h, an h below 4, a size > 32767 or a w < 1, an
 * unknown layout or pixel format, a null table, an offset outside its range, or a matrix the rules above do not admit.  All of these are
 * refused before a device is touched.  When it fails *out_plan is NULL and crtfx_field420_last_error(NULL) holds the message (per calling
 * thread).  The chroma of a new plan is CRTFX_FIELD420_REPLICATE. */
int crtfx_field420_create(int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, crtfx_field420** out_plan);
int crtfx_field420_destroy(crtfx_field420* plan);
const char* crtfx_field420_last_error(const crtfx_field420* plan);

/* The bytes of one SOURCE frame (the layout's expression above); 0 for a null plan. */
size_t crtfx_field420_frame_bytes(const crtfx_field420* plan);

/* n frames in one call: frame i is read at src_base + i * src_stride_bytes (frame_bytes bytes) and written at
 * dst_base + i * dst_stride_bytes (h x w x 3 bytes or halves, rows unpadded); strides of at least a frame.  The 8-bit layouts take any
 * byte base and stride; the 10-bit ones need even bases and strides (CRTFX_E_INVALID otherwise).  Bytes between frames are neither read
 * nor written.  Source and destination must not overlap. */
int crtfx_field420_run(crtfx_field420* plan, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream);

/* FORCE_GENERAL (0 / 1): take the narrow-access kernel whatever the width and alignment.  CHROMA (CRTFX_FIELD420_REPLICATE / _LEFT /
 * _CENTER): how the runs that follow up-sample chroma inside a field; a live plan may be switched back and forth.  Any other option or
 * value: CRTFX_E_INVALID. */
typedef enum crtfx_field420_option { CRTFX_FIELD420_OPT_FORCE_GENERAL = 1, CRTFX_FIELD420_OPT_CHROMA = 2 } crtfx_field420_option;
int crtfx_field420_set_option(crtfx_field420* plan, int option, int value);

/* The path of the most recent crtfx_field420_run (before the first one: the path a run with aligned bases would take) and the chroma:
 * `field420=k_unpack_field420<nv12,vec>;chroma=left;frames=5` or `field420=k_unpack_field420<p010le,general>;chroma=replicate;frames=5`. */
int crtfx_field420_last_plan(crtfx_field420* plan, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* CRTFX_FIELD420_H */
