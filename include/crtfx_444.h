/*
 * crtfx_444.h — the 10-bit 4:4:4 pair of libcrtfx.so: full-resolution deep colour in front of and behind a chain that runs on half pixels
 * (CRTFX_PIX_F16, IEEE half on the 0..255 scale).  The source stage (crtfx_unpack444_*) converts yuv444p10le (ProRes 4444 / DNxHR 444
 * decodes), gbrp10le (DPX / TIFF / EXR sequences through ffmpeg) and x2rgb10le (10-bit screen and KMS capture) frames to h x w x 3 half RGB
 * frames on the device; the egress stage (crtfx_egress444_*) converts finished half RGB frames to the same formats.  No chroma sample is
 * dropped on either side — the 10-bit 4:2:0 pair (crtfx_deep.h) keeps one in four — and no host core touches a sample.  The two families
 * mirror crtfx_unpack10_* and crtfx_egress10_* function for function and refuse uint8 frames as those do.
 *
 * Status codes (crtfx_status), pixel formats (crtfx_pixfmt) and conventions are those of crtfx.h: the caller owns every frame; work is
 * enqueued on the caller's hipStream_t (void*, NULL = the default stream); only create / destroy synchronise; the calling thread's current
 * device must be the plan's when it runs.  Each stage has a handle of its own.
 *
 * Layouts: two memory layouts serve the three formats, which differ only in the table handed to create.  Rows are unpadded, words are
 * little-endian:
 *     CRTFX_444_PLANAR      three planes P0 | P1 | P2, each h x w 16-bit words        frame_bytes = 6 * h * w
 *                           sample = word & 1023 when read, word = v when written
 *                           yuv444p10le: P = Y, U, V;   gbrp10le: P = G, B, R
 *     CRTFX_444_X2RGB10LE   h x w 32-bit words, three fields per word                 frame_bytes = 4 * h * w
 *                           P0 = (word >> 20) & 1023, P1 = (word >> 10) & 1023, P2 = word & 1023; written as P0 << 20 | P1 << 10 | P2
 *                           x2rgb10le: P = R, G, B
 * The bits outside a sample (the top 6 of a planar word, the top 2 of a packed one) are ignored when read and written as 0.  RGB frames are
 * h x w x 3 halves, rows unpadded.  Bases and strides on the half side must be even; on the 10-bit side even for CRTFX_444_PLANAR and
 * multiples of 4 for CRTFX_444_X2RGB10LE.
 *
 * Arithmetic: crtfx_deep.h's quarter codes (q = 0..1020, the half value q / 4, exact) without a chroma index.  32-bit signed integers, 16
 * fractional bits.
 *     source   c_j    = P_j - off_j                                                                          j = 0, 1, 2
 *              q[k]   = clamp((m[k][0] * c_0 + m[k][1] * c_1 + m[k][2] * c_2 + (1 << 15)) >> 16, 0, 1020)    k = R, G, B
 *              out[k] = half(q[k] / 4)                                                                       exact: no rounding occurs
 *     egress   q      = rint_to_even(min(max(4 * float(half), 0), 1020)), NaN -> 0                           crtfx_deep.h's quantiser
 *              T_j    = clamp((m_j . q + (off_j << 16) + (1 << 15)) >> 16, 0, 1023)                          plane j / field j
 * The kernels clamp the source accumulator at 0 first, shift the non-negative rest logically and take an unsigned minimum; create admits
 * only egress matrices whose accumulators stay in [0, 2^31), so there the lower clamp never acts.
 *
 * Tables (pythoncrt_amd.tables): yuv444p10le takes rgb_matrix10 / yuv_matrix10 as they are (bt601 / bt709, tv / pc).  The two RGB formats
 * take rgb_scale10("gbr") / rgb_scale10("rgb"): full-range RGB, offsets 0, one constant on a (permuted) diagonal — K = 65344 =
 * floor(1020/1023 * 65536 + 0.5) on the way in (0 -> 0, 1023 -> 1020, every quarter code is reached), K' = 65729 =
 * floor(1023/1020 * 65536 + 0.5) on the way out (1020 -> 1023).  q -> v -> q is exact for 1018 of the 1021 codes: 510 * 1023 / 1020 = 511.5
 * is a true tie, and 510, 849 and 850 come back one higher.
 * NOT claimed: byte equality with libswscale.  What the tests hold the kernels to is the arithmetic above (tests/deep444_model.py).
 *
 * Paths, chosen per run and named by *_last_plan; both give the same bytes.
 *     vec       taken when w % 8 == 0 and both frame bases are multiples of 4, and with n > 1 both strides too.  One lane owns one row of 8
 *               columns: 3 x 16 bytes (planar) or 2 x 16 bytes (x2rgb10le) on the 10-bit side, 48 bytes of half RGB, all as dword-multiple
 *               accesses.  Consecutive lanes take consecutive column blocks; all n frames are one grid.
 *     general   any size: one lane per pixel, 16-bit loads and stores (32-bit ones on the x2rgb10le side); every output word is written
 *               by exactly one lane and nothing outside the frame is touched.  Also the A/B and test fallback (*_OPT_FORCE_GENERAL).
 * Registers (gfx950, as built; tests/test_deep444_tables.py reads them from the library, holds every build to 128 and these counts to the
 * built ones): k_unpack10_444 <planar,vec> 32, <x2rgb10le,vec> 34, <planar,general> 10, <x2rgb10le,general> 10 VGPRs;
 * k_egress10_444 <planar,vec> 32, <x2rgb10le,vec> 32, <planar,general> 15, <x2rgb10le,general> 11 VGPRs; no AGPRs, no LDS,
 * no scratch, no spills.
 */
#ifndef CRTFX_444_H
#define CRTFX_444_H

#include <stddef.h>
#include <stdint.h>

#include "crtfx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crtfx_unpack444 crtfx_unpack444;
typedef struct crtfx_egress444 crtfx_egress444;

typedef enum crtfx_444_layout { CRTFX_444_PLANAR = 0, CRTFX_444_X2RGB10LE = 1 } crtfx_444_layout;

/* ---- source: `layout` -> h x w half RGB ----
 * Plans the conversion on `device` (synchronises; the calling thread's current device is restored).  pix_fmt, the format of the RGB frames
 * written: CRTFX_PIX_F16; CRTFX_PIX_U8 is CRTFX_E_UNSUPPORTED (only half frames are written).  m: 9 integers (rows R, G, B over the columns
 * P0, P1, P2), off: 3 integers in 0..1023.  CRTFX_E_INVALID: a size < 1 or > 32767, an unknown layout or pixel format, a null table, an
 * offset outside 0..1023, or a matrix whose accumulators could leave int32: a row k with
 * (|m[k][0]| + |m[k][1]| + |m[k][2]|) * 1023 + 2^15 >= 2^31.  All of these are refused before a device is touched.  When it fails
 * *out_plan is NULL and crtfx_unpack444_last_error(NULL) holds the message (per calling thread). */
int crtfx_unpack444_create(int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, crtfx_unpack444** out_plan);
int crtfx_unpack444_destroy(crtfx_unpack444* plan);
const char* crtfx_unpack444_last_error(const crtfx_unpack444* plan);

/* 6 * h * w (planar) or 4 * h * w (x2rgb10le), the bytes of one SOURCE frame; 0 for a null plan. */
size_t crtfx_unpack444_frame_bytes(const crtfx_unpack444* plan);

/* n frames in one call: frame i is read at src_base + i * src_stride_bytes (frame_bytes bytes) and written at
 * dst_base + i * dst_stride_bytes (h x w x 3 halves, rows unpadded); strides of at least a frame.  dst_base and dst_stride_bytes must be
 * even; src_base and src_stride_bytes even (planar) or multiples of 4 (x2rgb10le); CRTFX_E_INVALID otherwise.  Bytes between frames are
 * neither read nor written.  Source and destination must not overlap. */
int crtfx_unpack444_run(crtfx_unpack444* plan, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n,
                        void* stream);

/* Testing / A-B switches of one plan.  FORCE_GENERAL (0 / 1): take the one-pixel-per-lane kernel whatever the width and alignment. */
typedef enum crtfx_unpack444_option { CRTFX_UNPACK444_OPT_FORCE_GENERAL = 1 } crtfx_unpack444_option;
int crtfx_unpack444_set_option(crtfx_unpack444* plan, int option, int value);

/* The path of the most recent crtfx_unpack444_run (before the first one: the path a run with aligned bases would take):
 * `unpack444=k_unpack10_444<planar,vec>;frames=5` or `unpack444=k_unpack10_444<x2rgb10le,general>;frames=5`. */
int crtfx_unpack444_last_plan(crtfx_unpack444* plan, char* buf, size_t n);

/* ---- egress: h x w half RGB -> `layout` ----
 * As crtfx_unpack444_create, with pix_fmt the format of the RGB frames read and m = rows T0, T1, T2 over the columns R, G, B.  The matrix
 * is CRTFX_E_INVALID when an accumulator could leave [0, 2^31) for q <= 1020: with K_j = (off_j << 16) + 2^15, a row whose negative
 * entries' sum * 1020 + K_j < 0 or whose positive entries' sum * 1020 + K_j >= 2^31.  crtfx_egress444_last_error(NULL) holds create's
 * message. */
int crtfx_egress444_create(int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, crtfx_egress444** out_plan);
int crtfx_egress444_destroy(crtfx_egress444* plan);
const char* crtfx_egress444_last_error(const crtfx_egress444* plan);

/* The bytes of one OUTPUT frame (the same expression); 0 for a null plan. */
size_t crtfx_egress444_frame_bytes(const crtfx_egress444* plan);

/* n frames in one call: frame i is read at src_base + i * src_stride_bytes (h x w x 3 halves, rows unpadded) and written at
 * dst_base + i * dst_stride_bytes (frame_bytes bytes); the rules of crtfx_unpack444_run with the two sides exchanged. */
int crtfx_egress444_run(crtfx_egress444* plan, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n,
                        void* stream);

typedef enum crtfx_egress444_option { CRTFX_EGRESS444_OPT_FORCE_GENERAL = 1 } crtfx_egress444_option;
int crtfx_egress444_set_option(crtfx_egress444* plan, int option, int value);

/* `egress444=k_egress10_444<planar,general>;frames=5` or `egress444=k_egress10_444<x2rgb10le,vec>;frames=5`. */
int crtfx_egress444_last_plan(crtfx_egress444* plan, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* CRTFX_444_H */
