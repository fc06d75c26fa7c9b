/*
 * crtfx_egress.h — the egress stage of libcrtfx.so: finished uint8 RGB frames converted on the device to the 4:2:0 layout an encoder
 * takes — planar yuv420p (I420) or semi-planar nv12 — the last step of the reference's render loop, where each of its three encoder
 * branches ends in `-pix_fmt yuv420p` (crt_filter.py ref:970-1002) and libswscale converts the rgb24 pipe on one host core.  A frame
 * leaves the device as 1.5 bytes per pixel instead of 3.
 *
 * Status codes (crtfx_status), pixel formats (crtfx_pixfmt) and conventions are those of crtfx.h and crtfx_ingest.h: the caller owns
 * every frame; work is enqueued on the caller's hipStream_t (void*, NULL = the default stream); only create / destroy synchronise; the
 * calling thread's current device must be the plan's when it runs.  The stage depends on a device, a size, a layout and an integer
 * matrix, not on a crtfx_ctx: it has a handle of its own.
 *
 * Layout.  With ch = (h + 1) / 2 and cw = (w + 1) / 2 a frame is frame_bytes = h * w + 2 * ch * cw bytes, every row unpadded:
 *     yuv420p   Y h x w | U ch x cw | V ch x cw
 *     nv12      Y h x w | UV ch x (2 * cw), U and V interleaved (U first)
 *
 * Arithmetic.  32-bit integers, 16 fractional bits; m = rows Y, U, V of a 3 x 3 integer matrix, off = (16 or 0, 128, 128):
 *     Y[y][x]   = clamp((m0 . rgb[y][x] + (off0 << 16) + (1 << 15)) >> 16, 0, 255)
 *     S[cy][cx] = rgb[y0][x0] + rgb[y0][x1] + rgb[y1][x0] + rgb[y1][x1]                                  per channel,
 *                 y0 = 2 cy, y1 = min(2 cy + 1, h - 1), x0 = 2 cx, x1 = min(2 cx + 1, w - 1)
 *     U[cy][cx] = clamp((m1 . S + (off1 << 18) + (1 << 17)) >> 18, 0, 255)
 *     V[cy][cx] = clamp((m2 . S + (off2 << 18) + (1 << 17)) >> 18, 0, 255)
 * Chroma is the conversion of the 2 x 2 box mean (centre siting); an odd edge replicates the last row / column.  The upper clamp is
 * live: at full range pure blue gives U = 256 and pure red V = 256 before it.  The matrices of pythoncrt_amd.tables.yuv_matrix
 * (BT.601 / BT.709, limited / full range) are floor(c * 65536 + 0.5) of the float64 expressions, the G entries then set so that the Y row
 * sums to floor(sy * 65536 + 0.5) and the chroma rows to 0 (every grey gives U = V = 128 exactly).  The default of the Python layer,
 * bt601 / limited, is the colourimetry libswscale applies to an untagged rgb24 -> yuv420p conversion.
 * NOT claimed: byte equality with libswscale.  Its 15-bit intermediate and its dither are not restated here, and no test depends on
 * ffmpeg; what the tests hold the kernels to is the arithmetic above (tests/yuv_model.py), to the byte.
 *
 * Paths, chosen per run and named by crtfx_egress_last_plan; both give the same bytes.
 *     vec       taken when w % 8 == 0 and the source and destination frame bases are 4-byte aligned: src_base and dst_base are
 *               multiples of 4, and with n > 1 so are both strides.  (Then every source row, every Y row and every chroma row starts on
 *               a 4-byte boundary: 3 w, w, w / 2 and h w + ch cw are multiples of 4.)  One lane owns 2 rows x 8 columns: it loads the
 *               2 x 24 source bytes as dwords, stores Y as two 8-byte stores and the four chroma pairs as one dword per plane (yuv420p)
 *               or one 8-byte store (nv12), each chroma sample computed from the registers that hold its four luma samples.  Consecutive
 *               lanes take consecutive column blocks; all n frames are one grid.  An odd h is served: the last lane row stores one Y row.
 *     general   any size, any byte alignment: one lane per chroma sample, byte loads and byte stores; each chroma sample (and each Y
 *               byte) is written by exactly one lane.  Also the A/B and test fallback (CRTFX_EGRESS_OPT_FORCE_GENERAL).
 */
#ifndef CRTFX_EGRESS_H
#define CRTFX_EGRESS_H

#include <stddef.h>
#include <stdint.h>

#include "crtfx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crtfx_egress crtfx_egress;

typedef enum crtfx_egress_layout { CRTFX_EGRESS_YUV420P = 0, CRTFX_EGRESS_NV12 = 1 } crtfx_egress_layout;

/* Plans h x w RGB -> `layout` on `device` (synchronises; the calling thread's current device is restored).  pix_fmt: CRTFX_PIX_U8;
 * CRTFX_PIX_F16 is CRTFX_E_UNSUPPORTED.  m: 9 integers (rows Y, U, V), off: 3 integers in 0..255.  CRTFX_E_INVALID: a size < 1 or
 * > 32767, an unknown layout or pixel format, a null table, an offset outside 0..255, or a matrix whose accumulators could leave
 * [0, 2^31): per row, with P / N the sums of its positive / negative entries and X = 255 (Y row) or 1020 (chroma rows), the constant
 * term + N * X must be >= 0 and the constant term + P * X < 2^31.  When it fails *out_plan is NULL and crtfx_egress_last_error(NULL)
 * holds the message (per calling thread). */
int crtfx_egress_create(int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, crtfx_egress** out_plan);
int crtfx_egress_destroy(crtfx_egress* plan);
const char* crtfx_egress_last_error(const crtfx_egress* plan);

/* h * w + 2 * ((h + 1) / 2) * ((w + 1) / 2); 0 for a null plan. */
size_t crtfx_egress_frame_bytes(const crtfx_egress* plan);

/* n frames in one call: frame i is read at src_base + i * src_stride_bytes (h x w x 3 uint8, rows unpadded) and written at
 * dst_base + i * dst_stride_bytes (frame_bytes bytes); strides of at least a frame, any byte alignment.  Bytes between frames are
 * neither read nor written.  Source and destination must not overlap. */
int crtfx_egress_run(crtfx_egress* plan, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n,
                     void* stream);

/* Testing / A-B switches of one plan.  FORCE_GENERAL (0 / 1): take the byte-access kernel whatever the width and alignment. */
typedef enum crtfx_egress_option { CRTFX_EGRESS_OPT_FORCE_GENERAL = 1 } crtfx_egress_option;
int crtfx_egress_set_option(crtfx_egress* plan, int option, int value);

/* The path of the most recent crtfx_egress_run (before the first one: the path a run with aligned bases would take), in the style of
 * crtfx_last_plan: `egress=k_egress_420<nv12,vec>;frames=5` or `egress=k_egress_420<yuv420p,general>;frames=5`. */
int crtfx_egress_last_plan(crtfx_egress* plan, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* CRTFX_EGRESS_H */
