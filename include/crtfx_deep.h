/*
 * crtfx_deep.h — the 10-bit pair of libcrtfx.so: what stands in front of and behind a chain that runs on half pixels (CRTFX_PIX_F16, IEEE
 * half on the 0..255 scale).  The source stage (crtfx_unpack10_*) converts the 10-bit 4:2:0 frames a decoder hands out — planar yuv420p10le
 * (software decoders) or semi-planar p010le (hardware decoders) — to h x w x 3 half RGB frames on the device; the egress stage
 * (crtfx_egress10_*) converts finished half RGB frames to the same two layouts for an encoder.  A 10-bit stream then crosses the pipe, the
 * pinned slot and PCIe as 3 bytes per pixel each way instead of the 6 of raw half RGB, and no host core touches a sample.  The two families
 * mirror crtfx_unpack_* (crtfx_unpack.h) and crtfx_egress_* (crtfx_egress.h) function for function; the 8-bit stages keep refusing half
 * frames, these refuse uint8 ones.
 *
 * Status codes (crtfx_status), pixel formats (crtfx_pixfmt) and conventions are those of crtfx.h: the caller owns every frame; work is
 * enqueued on the caller's hipStream_t (void*, NULL = the default stream); only create / destroy synchronise; the calling thread's current
 * device must be the plan's when it runs.  Each stage has a handle of its own.
 *
 * Layouts: the geometry of the 8-bit stages with 16-bit little-endian words instead of bytes.  With ch = (h + 1) / 2 and cw = (w + 1) / 2
 * a frame is frame_bytes = 2 * (h * w + 2 * ch * cw) bytes, every row unpadded (what ffmpeg's rawvideo reads and writes, odd sizes included):
 *     yuv420p10le   Y h x w | U ch x cw | V ch x cw                       sample = word & 1023 when read, word = v when written
 *     p010le        Y h x w | UV ch x (2 * cw), U and V interleaved       sample = word >> 6 when read,   word = v << 6 when written
 * The bits of a word outside its sample are ignored when read and written as 0.  RGB frames are h x w x 3 halves, rows unpadded.  Every
 * frame base and frame stride must be even.
 *
 * Quarter codes.  The stages meet the chain in "quarter codes" q = 0..1020, the half value q / 4 on the 0..255 scale: 10-bit limited-range
 * white (940) is q = 1020 is 255.0.  Every quarter code is exactly a half (spacing 0.25; half's spacing below 256 is at most 0.125), so
 * both directions are integer arithmetic with one stated rounding, and the tests hold every kernel build to an int64 model bit for bit.
 *
 * Source arithmetic.  32-bit signed integers, 16 fractional bits; m = rows R, G, B of a 3 x 3 integer matrix over the columns (Y, U, V),
 * off = (64 or 0, 512, 512):
 *     c = Y[y][x] - off0      d = U[y >> 1][x >> 1] - off1      e = V[y >> 1][x >> 1] - off2
 *     q[k]   = clamp((m[k][0] * c + m[k][1] * d + m[k][2] * e + (1 << 15)) >> 16, 0, 1020)               k = R, G, B
 *     out[k] = half(q[k] / 4)                                                                             exact: no rounding occurs
 * Chroma is replicated over its 2 x 2 block (the inverse siting of the egress stage's box mean); an odd edge reads the last chroma sample.
 * Both clamps are live, as in crtfx_unpack.h; the kernels clamp the accumulator at 0 first and shift the non-negative rest.
 *
 * Egress arithmetic.  m = rows Y, U, V; off = (64 or 0, 512, 512):
 *     f = float(half)      q = rint_to_even(min(max(4 f, 0), 1020)), NaN -> 0         (so -0, negatives, -inf -> 0; +inf -> 1020)
 *     Y[y][x]   = clamp((m0 . q[y][x] + (off0 << 16) + (1 << 15)) >> 16, 0, 1023)
 *     S[cy][cx] = q[y0][x0] + q[y0][x1] + q[y1][x0] + q[y1][x1]        y0 = 2 cy, x0 = 2 cx, y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1)
 *     U[cy][cx] = clamp((m1 . S + (512 << 18) + (1 << 17)) >> 18, 0, 1023)            V likewise with m2 (with off1, off2 for 512)
 * The half -> float conversion and 4 f are exact; the single rounding is the rint.  create admits only matrices whose accumulators stay in
 * [0, 2^31), so the lower clamp never acts.
 *
 * The matrices of pythoncrt_amd.tables.rgb_matrix10 / yuv_matrix10 follow the recipes of rgb_matrix / yuv_matrix (floor(c * 65536 + 0.5) of
 * the float64 expressions; yuv_matrix10 with the same G-entry adjustment) on the scales of quarter codes: source sy' = 1020/876 and
 * sc' = 1020/896 (limited) or both 1020/1023 (full); egress sy = 876/1020 and sc = 896/1020 (limited) or both 1023/1020 (full).  10-bit
 * limited range is exactly 4 x the 8-bit one, so the limited-range matrices are those of the 8-bit stages.
 * NOT claimed: byte equality with libswscale.  What the tests hold the kernels to is the arithmetic above (tests/deep_model.py).
 *
 * Paths, chosen per run and named by *_last_plan; both give the same bytes.
 *     vec       taken when w % 8 == 0 and the frame bases are 4-byte aligned: src_base and dst_base are multiples of 4, and with n > 1 so
 *               are both strides (the 8-bit stages' rule; every row and plane then starts on a 4-byte boundary).  One lane owns 2 rows x 8
 *               columns: 2 x 16 bytes of Y, 2 x 8 (yuv420p10le) or 16 (p010le) bytes of chroma, 2 x 48 bytes of half RGB, all as
 *               dword-multiple accesses; each chroma term is formed once for the four pixels under it.  Consecutive lanes take consecutive
 *               column blocks; all n frames are one grid.  An odd h is served: the last lane row loads and stores one row.
 *     general   any size: one lane per chroma sample, 16-bit loads and stores; every output word is written by exactly one lane, and
 *               nothing beyond x < w, y < h is read or written at an odd edge.  Also the A/B and test fallback (*_OPT_FORCE_GENERAL).
 * Registers (gfx950, as built; tests/test_deep_tables.py reads them from the library and holds every build to 128, four waves per SIMD):
 * k_unpack10_420_vec 45 VGPRs, k_unpack10_420_general 18, k_egress10_420_vec 71 (yuv420p10le) / 70 (p010le), k_egress10_420_general 21;
 * no AGPRs, no LDS, no scratch, no spills.  The egress vec kernel holds 2 x 12 input dwords and so passes 64: seven waves per SIMD instead
 * of eight (forcing 64 spills four registers; a 2 x 4 lane would fit and halve the bytes per access).  Measured at 4K and 8K it runs at 0.83 - 0.91
 * of the time of a device-to-device copy of equal traffic (profiles/deep_yuv.txt), so it is left as it is.
 */
#ifndef CRTFX_DEEP_H
#define CRTFX_DEEP_H

#include <stddef.h>
#include <stdint.h>

#include "crtfx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crtfx_unpack10 crtfx_unpack10;
typedef struct crtfx_egress10 crtfx_egress10;

typedef enum crtfx_deep_layout { CRTFX_DEEP_YUV420P10LE = 0, CRTFX_DEEP_P010LE = 1 } crtfx_deep_layout;

/* ---- source: `layout` -> h x w half RGB ----
 * Plans the conversion on `device` (synchronises; the calling thread's current device is restored).  pix_fmt, the format of the RGB frames
 * written: CRTFX_PIX_F16; CRTFX_PIX_U8 is CRTFX_E_UNSUPPORTED (only half frames are written).  m: 9 integers (rows R, G, B over the columns
 * Y, U, V), off: 3 integers in 0..1023.  CRTFX_E_INVALID: a size < 1 or > 32767, an unknown layout or pixel format, a null table, an offset
 * outside 0..1023, or a matrix whose accumulators could leave int32: a row k with (|m[k][0]| + |m[k][1]| + |m[k][2]|) * 1023 + 2^15 >= 2^31.
 * All of these are refused before a device is touched.  When it fails *out_plan is NULL and crtfx_unpack10_last_error(NULL) holds the
 * message (per calling thread). */
int crtfx_unpack10_create(int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, crtfx_unpack10** out_plan);
int crtfx_unpack10_destroy(crtfx_unpack10* plan);
const char* crtfx_unpack10_last_error(const crtfx_unpack10* plan);

/* 2 * (h * w + 2 * ((h + 1) / 2) * ((w + 1) / 2)), the bytes of one SOURCE frame; 0 for a null plan. */
size_t crtfx_unpack10_frame_bytes(const crtfx_unpack10* plan);

/* n frames in one call: frame i is read at src_base + i * src_stride_bytes (frame_bytes bytes) and written at
 * dst_base + i * dst_stride_bytes (h x w x 3 halves, rows unpadded); strides of at least a frame.  Bases and strides must be even
 * (CRTFX_E_INVALID otherwise).  Bytes between frames are neither read nor written.  Source and destination must not overlap. */
int crtfx_unpack10_run(crtfx_unpack10* plan, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n,
                       void* stream);

/* Testing / A-B switches of one plan.  FORCE_GENERAL (0 / 1): take the 16-bit-access kernel whatever the width and alignment. */
typedef enum crtfx_unpack10_option { CRTFX_UNPACK10_OPT_FORCE_GENERAL = 1 } crtfx_unpack10_option;
int crtfx_unpack10_set_option(crtfx_unpack10* plan, int option, int value);

/* The path of the most recent crtfx_unpack10_run (before the first one: the path a run with aligned bases would take):
 * `unpack10=k_unpack10_420<p010le,vec>;frames=5` or `unpack10=k_unpack10_420<yuv420p10le,general>;frames=5`. */
int crtfx_unpack10_last_plan(crtfx_unpack10* plan, char* buf, size_t n);

/* ---- egress: h x w half RGB -> `layout` ----
 * As crtfx_unpack10_create, with pix_fmt the format of the RGB frames read and m = rows Y, U, V over the columns R, G, B.  The matrix is
 * CRTFX_E_INVALID when an accumulator could leave [0, 2^31) for q <= 1020 and S <= 4080: with K0 = (off0 << 16) + 2^15 and
 * K1,2 = (off1,2 << 18) + 2^17, a row whose negative entries' sum * X + K < 0 or whose positive entries' sum * X + K >= 2^31 (X = 1020 for
 * the Y row, 4080 for the chroma rows).  crtfx_egress10_last_error(NULL) holds create's message. */
int crtfx_egress10_create(int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, crtfx_egress10** out_plan);
int crtfx_egress10_destroy(crtfx_egress10* plan);
const char* crtfx_egress10_last_error(const crtfx_egress10* plan);

/* The bytes of one OUTPUT frame (the same expression); 0 for a null plan. */
size_t crtfx_egress10_frame_bytes(const crtfx_egress10* plan);

/* n frames in one call: frame i is read at src_base + i * src_stride_bytes (h x w x 3 halves, rows unpadded) and written at
 * dst_base + i * dst_stride_bytes (frame_bytes bytes); the rules of crtfx_unpack10_run. */
int crtfx_egress10_run(crtfx_egress10* plan, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n,
                       void* stream);

typedef enum crtfx_egress10_option { CRTFX_EGRESS10_OPT_FORCE_GENERAL = 1 } crtfx_egress10_option;
int crtfx_egress10_set_option(crtfx_egress10* plan, int option, int value);

/* `egress10=k_egress10_420<yuv420p10le,general>;frames=5` or `egress10=k_egress10_420<p010le,vec>;frames=5`. */
int crtfx_egress10_last_plan(crtfx_egress10* plan, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* CRTFX_DEEP_H */
