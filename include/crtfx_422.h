/*
 * crtfx_422.h — the 8-bit 4:2:2 pair of libcrtfx.so: the source stage (crtfx_unpack422_*) converts the uint8 4:2:2 frames a capture card
 * (uyvy422 / yuyv422) or a mezzanine decoder (yuv422p) hands out to the uint8 h x w x 3 RGB frames the effect chain takes; the egress stage
 * (crtfx_egress422_*) converts finished uint8 RGB frames to the same three layouts.  A 4:2:2 stream then crosses the pipe, the pinned slot
 * and PCIe as 2 bytes per pixel instead of the 3 of rgb24, no `-pix_fmt rgb24` / `-pix_fmt yuv420p` conversion (libswscale, one host core)
 * stands at either end, and the vertical chroma resolution the source had is kept on the way out.  The two families mirror crtfx_unpack_*
 * (crtfx_unpack.h) and crtfx_egress_* (crtfx_egress.h) function for function; those keep serving 4:2:0 only.
 *
 * Status codes (crtfx_status), pixel formats (crtfx_pixfmt) and conventions are those of crtfx.h: the caller owns every frame; work is
 * enqueued on the caller's hipStream_t (void*, NULL = the default stream); only create / destroy synchronise; the calling thread's current
 * device must be the plan's when it runs.  Each stage has a handle of its own.
 *
 * Layouts.  With cw = (w + 1) / 2, every row unpadded, sizes 1..32767 (odd ones included):
 *     yuv422p   Y h x w | U h x cw | V h x cw                       frame_bytes = h * w + 2 * h * cw
 *     yuyv422   h rows of cw macropixels  Y0 U Y1 V                  frame_bytes = 4 * h * cw
 *     uyvy422   h rows of cw macropixels  U Y0 V Y1                  frame_bytes = 4 * h * cw
 * For an even w these are the formats' definitions and 4 * cw = 2 * w.  For an odd w the last macropixel of a packed row has no second
 * pixel: its Y1 byte is padding, ignored when read and written as a copy of the row's last Y (so every output byte is defined).  That is
 * this library's rule, not a claim about any other program.  RGB frames are h x w x 3 uint8, rows unpadded.
 *
 * Source arithmetic: that of crtfx_unpack.h with one index changed.  32-bit signed integers, 16 fractional bits; m = rows R, G, B of a
 * 3 x 3 integer matrix over the columns (Y, U, V), off = (16 or 0, 128, 128) — exactly what pythoncrt_amd.tables.rgb_matrix returns:
 *     c = Y[y][x] - off0      d = U[y][x >> 1] - off1      e = V[y][x >> 1] - off2
 *     out[y][x][k] = clamp((m[k][0] * c + m[k][1] * d + m[k][2] * e + (1 << 15)) >> 16, 0, 255)          k = R, G, B
 * Chroma is replicated over its horizontal pair; an odd edge reads the last sample.  Both clamps are live; the kernels clamp the
 * accumulator at 0 first, shift the non-negative rest logically and take an unsigned minimum (see crtfx_unpack.hip for the reason).
 *
 * Egress arithmetic.  m = rows Y, U, V over the columns (R, G, B), off = (16 or 0, 128, 128) — what tables.yuv_matrix returns:
 *     Y[y][x]  = clamp((m0 . rgb[y][x] + (off0 << 16) + (1 << 15)) >> 16, 0, 255)                        the 4:2:0 stage's Y, unchanged
 *     S[y][cx] = rgb[y][x0] + rgb[y][x1]                  x0 = 2 cx, x1 = min(2 cx + 1, w - 1)
 *     U[y][cx] = clamp((m1 . S + (off1 << 17) + (1 << 16)) >> 17, 0, 255)                                V likewise with m2, off2
 * The horizontal pair mean: a uniform pair has the per-pixel chroma, and every grey gives 128 / 128 because the chroma rows sum to 0.
 * create admits only matrices whose accumulators stay in [0, 2^31), so the lower clamp never acts; the upper one is live (full range,
 * pure blue's U is 256 before it).
 * NOT claimed: byte equality with libswscale.  What the tests hold the kernels to is the arithmetic above (tests/yuv422_model.py).
 *
 * Paths, chosen per run and named by *_last_plan; both give the same bytes.  Kernels: k_unpack_422<layout, path> and
 * k_egress_422<layout, path> in namespace crtfx_422_impl, twelve builds.
 *     vec       taken when w % 8 == 0 and the frame bases are 4-byte aligned: src_base and dst_base are multiples of 4, and with n > 1 so
 *               are both strides.  (Then every row and every plane starts on a 4-byte boundary: w, w / 2, h w, h cw, 2 w and 3 w are
 *               multiples of 4.)  One lane owns one row of 8 columns: the packed layouts' 16 bytes are one 16-byte access; yuv422p's are
 *               8 Y bytes as one 8-byte access and one dword per chroma plane; the 24 RGB bytes are 16 + 8 bytes.  Each chroma term is
 *               formed once per pair.  Consecutive lanes take consecutive column blocks of a row, rows follow each other, and all n frames
 *               are one grid.  Stores are plain ones, as in the 4:2:0 stages.
 *     general   any size, any byte alignment: one lane per chroma sample (per macropixel), byte loads and byte stores; every output byte
 *               is written by exactly one lane — the pad byte of an odd-width packed row included — and nothing beyond the frame is read
 *               or written.  Also the A/B and test fallback (*_OPT_FORCE_GENERAL).
 * Every build uses no LDS, no scratch, no spills and at most 64 VGPRs + AGPRs (tests/test_yuv422_tables.py reads them from the library).
 */
#ifndef CRTFX_422_H
#define CRTFX_422_H

#include <stddef.h>
#include <stdint.h>

#include "crtfx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crtfx_unpack422 crtfx_unpack422;
typedef struct crtfx_egress422 crtfx_egress422;

typedef enum crtfx_422_layout { CRTFX_422_YUV422P = 0, CRTFX_422_YUYV422 = 1, CRTFX_422_UYVY422 = 2 } crtfx_422_layout;

/* ---- source: `layout` -> h x w RGB ----
 * Plans the conversion on `device` (synchronises; the calling thread's current device is restored).  pix_fmt, the format of the RGB frames
 * written: CRTFX_PIX_U8; CRTFX_PIX_F16 is CRTFX_E_UNSUPPORTED (only uint8 frames are written).  m: 9 integers (rows R, G, B over the columns
 * Y, U, V), off: 3 integers in 0..255.  CRTFX_E_INVALID: a size < 1 or > 32767, an unknown layout or pixel format, a null table, an offset
 * outside 0..255, or a matrix whose accumulators could leave int32: a row k with (|m[k][0]| + |m[k][1]| + |m[k][2]|) * 255 + 2^15 >= 2^31
 * (the rule of crtfx_unpack_create).  All of these are refused before a device is touched.  When it fails *out_plan is NULL and
 * crtfx_unpack422_last_error(NULL) holds the message (per calling thread). */
int crtfx_unpack422_create(int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, crtfx_unpack422** out_plan);
int crtfx_unpack422_destroy(crtfx_unpack422* plan);
const char* crtfx_unpack422_last_error(const crtfx_unpack422* plan);

/* The bytes of one SOURCE frame (see Layouts); 0 for a null plan. */
size_t crtfx_unpack422_frame_bytes(const crtfx_unpack422* plan);

/* n frames in one call: frame i is read at src_base + i * src_stride_bytes (frame_bytes bytes) and written at
 * dst_base + i * dst_stride_bytes (h x w x 3 uint8, rows unpadded); strides of at least a frame, any byte alignment.  Bytes between frames
 * are neither read nor written.  Source and destination must not overlap. */
int crtfx_unpack422_run(crtfx_unpack422* plan, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n,
                        void* stream);

/* Testing / A-B switches of one plan.  FORCE_GENERAL (0 / 1): take the byte-access kernel whatever the width and alignment. */
typedef enum crtfx_unpack422_option { CRTFX_UNPACK422_OPT_FORCE_GENERAL = 1 } crtfx_unpack422_option;
int crtfx_unpack422_set_option(crtfx_unpack422* plan, int option, int value);

/* The path of the most recent crtfx_unpack422_run (before the first one: the path a run with aligned bases would take):
 * `unpack422=k_unpack_422<uyvy422,vec>;frames=5` or `unpack422=k_unpack_422<yuv422p,general>;frames=5`. */
int crtfx_unpack422_last_plan(crtfx_unpack422* plan, char* buf, size_t n);

/* ---- egress: h x w RGB -> `layout` ----
 * As crtfx_unpack422_create, with pix_fmt the format of the RGB frames read and m = rows Y, U, V over the columns R, G, B.  The matrix is
 * CRTFX_E_INVALID when an accumulator could leave [0, 2^31) for a sample <= 255 and S <= 510: with K0 = (off0 << 16) + 2^15 and
 * K1,2 = (off1,2 << 17) + 2^16, a row whose negative entries' sum * X + K < 0 or whose positive entries' sum * X + K >= 2^31 (X = 255 for
 * the Y row, 510 for the chroma rows).  crtfx_egress422_last_error(NULL) holds create's message. */
int crtfx_egress422_create(int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, crtfx_egress422** out_plan);
int crtfx_egress422_destroy(crtfx_egress422* plan);
const char* crtfx_egress422_last_error(const crtfx_egress422* plan);

/* The bytes of one OUTPUT frame (the same expression); 0 for a null plan. */
size_t crtfx_egress422_frame_bytes(const crtfx_egress422* plan);

/* n frames in one call: frame i is read at src_base + i * src_stride_bytes (h x w x 3 uint8, rows unpadded) and written at
 * dst_base + i * dst_stride_bytes (frame_bytes bytes); the rules of crtfx_unpack422_run. */
int crtfx_egress422_run(crtfx_egress422* plan, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n,
                        void* stream);

typedef enum crtfx_egress422_option { CRTFX_EGRESS422_OPT_FORCE_GENERAL = 1 } crtfx_egress422_option;
int crtfx_egress422_set_option(crtfx_egress422* plan, int option, int value);

/* `egress422=k_egress_422<yuyv422,vec>;frames=5` or `egress422=k_egress_422<yuv422p,general>;frames=5`. */
int crtfx_egress422_last_plan(crtfx_egress422* plan, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* CRTFX_422_H */
