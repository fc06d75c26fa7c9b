/*
 * crtfx_unpack.h — the source stage of libcrtfx.so: uint8 frames in the 4:2:0 layout a decoder hands out — planar yuv420p (I420, software
 * decoders) or semi-planar nv12 (hardware decoders) — converted on the device to the uint8 h x w x 3 RGB frames the effect chain takes.
 * The mirror image of the egress stage (crtfx_egress.h): a frame reaches the device as 1.5 bytes per pixel instead of 3, and no
 * `-pix_fmt rgb24` conversion (libswscale, one host core) stands in front of the reader.
 *
 * Status codes (crtfx_status), pixel formats (crtfx_pixfmt) and conventions are those of crtfx.h, crtfx_ingest.h and crtfx_egress.h: the
 * caller owns every frame; work is enqueued on the caller's hipStream_t (void*, NULL = the default stream); only create / destroy
 * synchronise; the calling thread's current device must be the plan's when it runs.  The stage depends on a device, a size, a layout and an
 * integer matrix, not on a crtfx_ctx: it has a handle of its own.
 *
 * Layout: that of crtfx_egress.h, read instead of written.  With ch = (h + 1) / 2 and cw = (w + 1) / 2 a frame is
 * frame_bytes = h * w + 2 * ch * cw bytes, every row unpadded (what ffmpeg's rawvideo writes, odd sizes included):
 *     yuv420p   Y h x w | U ch x cw | V ch x cw
 *     nv12      Y h x w | UV ch x (2 * cw), U and V interleaved (U first)
 *
 * Arithmetic.  32-bit signed integers, 16 fractional bits; m = rows R, G, B of a 3 x 3 integer matrix over the columns (Y, U, V),
 * off = (16 or 0, 128, 128):
 *     c = Y[y][x] - off0      d = U[y >> 1][x >> 1] - off1      e = V[y >> 1][x >> 1] - off2
 *     out[y][x][k] = clamp((m[k][0] * c + m[k][1] * d + m[k][2] * e + (1 << 15)) >> 16, 0, 255)          k = R, G, B
 * Chroma is replicated over its 2 x 2 block: the inverse siting of the egress stage's box mean, and what libswscale's default unscaled
 * yuv420p -> rgb24 converter does.  Bilinear chroma up-sampling is out of scope.  An odd edge reads the last chroma sample.
 * Both clamps are live: limited-range white with V = 240 exceeds 255 in R, and Y = 16, U = V = 16 is negative in R and B (U = V = 240 in
 * G).  The accumulator can be negative; whatever sits below a negative quotient clamps to 0, so an arithmetic (floor) and a truncating
 * shift give the same bytes — the kernels clamp the accumulator at 0 first and shift the non-negative rest.  Neither form is "more
 * right": leave it.
 * The matrices of pythoncrt_amd.tables.rgb_matrix (BT.601 / BT.709, limited / full range) are floor(c * 65536 + 0.5) of the float64
 * expressions, with kg = 1 - kr - kb, sy' = 255/219 and sc' = 255/224 (limited) or 1 (full):
 *     Y column (all three rows) sy'      R,V 2 (1 - kr) sc'      G,U -2 kb (1 - kb) / kg sc'      G,V -2 kr (1 - kr) / kg sc'
 *     B,U 2 (1 - kb) sc'                 R,U and B,V exactly 0
 * No entry is adjusted afterwards; the three Y entries are one number, so every grey (U = V = 128) gives R = G = B.
 * NOT claimed: byte equality with libswscale (its tables and dither are not restated here, and no test depends on ffmpeg); what the tests
 * hold the kernels to is the arithmetic above (tests/unpack_model.py), to the byte.
 *
 * Paths, chosen per run and named by crtfx_unpack_last_plan; both give the same bytes.
 *     vec       taken when w % 8 == 0 and the source and destination frame bases are 4-byte aligned: src_base and dst_base are
 *               multiples of 4, and with n > 1 so are both strides.  (Then every Y row, every chroma row, every plane start and every
 *               RGB row starts on a 4-byte boundary: w, w / 2, h w, ch cw and 3 w are multiples of 4.)  One lane owns 2 rows x 8 columns:
 *               it loads the 2 x 8 Y bytes as two 8-byte loads and the 4 U and 4 V bytes as one dword per plane (yuv420p) or one 8-byte
 *               load (nv12), forms each chroma term m[k][1] * d + m[k][2] * e once per chroma sample for the four pixels under it, and
 *               stores the 2 x 24 RGB bytes as 16 + 8 bytes per row.  Consecutive lanes take consecutive column blocks; all n frames are
 *               one grid.  An odd h is served: the last lane row loads and stores one row.
 *     general   any size, any byte alignment: one lane per chroma sample, byte loads and byte stores; each RGB byte is written by exactly
 *               one lane, and nothing beyond x < w, y < h is read or written at an odd edge.  Also the A/B and test fallback
 *               (CRTFX_UNPACK_OPT_FORCE_GENERAL).
 */
#ifndef CRTFX_UNPACK_H
#define CRTFX_UNPACK_H

#include <stddef.h>
#include <stdint.h>

#include "crtfx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crtfx_unpack crtfx_unpack;

typedef enum crtfx_unpack_layout { CRTFX_UNPACK_YUV420P = 0, CRTFX_UNPACK_NV12 = 1 } crtfx_unpack_layout;

/* Plans `layout` -> h x w RGB on `device` (synchronises; the calling thread's current device is restored).  pix_fmt, the format of the RGB
 * frames written: CRTFX_PIX_U8; CRTFX_PIX_F16 is CRTFX_E_UNSUPPORTED.  m: 9 integers (rows R, G, B over the columns Y, U, V), off: 3
 * integers in 0..255.  CRTFX_E_INVALID: a size < 1 or > 32767, an unknown layout or pixel format, a null table, an offset outside 0..255,
 * or a matrix whose accumulators could leave int32: a row k with |m[k][0]| * 255 + |m[k][1]| * 255 + |m[k][2]| * 255 + 2^15 >= 2^31.  All
 * of these are refused before a device is touched.  When it fails *out_plan is NULL and crtfx_unpack_last_error(NULL) holds the message
 * (per calling thread). */
int crtfx_unpack_create(int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, crtfx_unpack** out_plan);
int crtfx_unpack_destroy(crtfx_unpack* plan);
const char* crtfx_unpack_last_error(const crtfx_unpack* plan);

/* h * w + 2 * ((h + 1) / 2) * ((w + 1) / 2), the bytes of one SOURCE frame; 0 for a null plan. */
size_t crtfx_unpack_frame_bytes(const crtfx_unpack* plan);

/* n frames in one call: frame i is read at src_base + i * src_stride_bytes (frame_bytes bytes) and written at
 * dst_base + i * dst_stride_bytes (h x w x 3 uint8, rows unpadded); strides of at least a frame, any byte alignment.  Bytes between frames
 * are neither read nor written.  Source and destination must not overlap. */
int crtfx_unpack_run(crtfx_unpack* plan, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n,
                     void* stream);

/* Testing / A-B switches of one plan.  FORCE_GENERAL (0 / 1): take the byte-access kernel whatever the width and alignment. */
typedef enum crtfx_unpack_option { CRTFX_UNPACK_OPT_FORCE_GENERAL = 1 } crtfx_unpack_option;
int crtfx_unpack_set_option(crtfx_unpack* plan, int option, int value);

/* The path of the most recent crtfx_unpack_run (before the first one: the path a run with aligned bases would take), in the style of
 * crtfx_last_plan: `unpack=k_unpack_420<nv12,vec>;frames=5` or `unpack=k_unpack_420<yuv420p,general>;frames=5`. */
int crtfx_unpack_last_plan(crtfx_unpack* plan, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* CRTFX_UNPACK_H */
