/*
 * crtfx_ingest.h — the ingest stage of libcrtfx.so: uint8 RGB frames of one size resized on the device to another,
 * byte for byte as Pillow's `Image.resize((w, h), Image.BILINEAR)` does it — the first step of the reference's render
 * loop, `Image.fromarray(frame).resize((out_w, out_h), Image.BILINEAR)` (crt_filter.py ref:1039-1041), for sources
 * that are not at the output size.
 *
 * Status codes (crtfx_status), pixel formats (crtfx_pixfmt) and conventions are those of crtfx.h: the caller owns every
 * frame; work is enqueued on the caller's hipStream_t (void*, NULL = the default stream); only create / destroy
 * synchronise; the calling thread's current device must be the plan's when it runs.  The stage depends on a device, two
 * sizes and two coefficient tables, not on a crtfx_ctx: it has a handle of its own.
 *
 * Arithmetic (Pillow's 8-bit resampler, src/libImaging/Resample.c): a pass along one axis computes
 *     out[xx] = clamp((2^21 + sum_{t < count[xx]} k[xx][t] * in[xmin[xx] + t]) >> 22, 0, 255)
 * in 32-bit integers; the horizontal pass runs first, its result is ROUNDED TO uint8, and the vertical pass reads that
 * uint8 image (so the two passes cannot be contracted into one 2-D sum).  The tables are HOST arrays built with Pillow's
 * float64 expressions (pythoncrt_amd.tables.pil_resample_axis) and copied by crtfx_ingest_create: per output index the
 * first tap `min`, the tap count `count` (1 <= count <= ksize, min + count <= n_in, both non-decreasing) and `ksize`
 * non-negative coefficients of at most 2^22 + ... < 2^24.
 *
 * Paths.  k_ingest_fused: one block per tile of output rows x output columns; the source rows and columns the tile's
 * taps reach are staged in LDS, the horizontal pass writes its uint8 result to LDS, the vertical pass reads it from
 * there.  It serves every size pair for which some tile shape of
 *     (rows, columns) in (32,128) (32,64) (16,128) (16,64) (8,64) (8,32) (4,32)        — the first that fits is taken —
 * has a footprint of at most 40 960 bytes of LDS (four blocks per CU), where, over all tiles of that shape,
 *     footprint = 4 * (2 * cols + cols * x_ksize + 2 * rows + rows * y_ksize)                      the tile's tables
 *               + max_source_rows * (round4(3 * max_source_cols + 3) + round4(3 * cols) + 4)       staged source + horizontal result
 * (cols / rows clipped to the output size).  That holds for every up-scale and for every ratio down to 1/4 on both
 * axes ((8,32): 40 source rows x (412 + 100) bytes), and for stronger reductions of small images.  Everything else — the
 * tap count grows with the down-scale factor without bound — takes the general path: k_ingest_h writes the horizontal
 * pass to a uint8 src_h x dst_w x 3 scratch the plan owns, k_ingest_v runs the vertical pass over it.
 */
#ifndef CRTFX_INGEST_H
#define CRTFX_INGEST_H

#include <stddef.h>
#include <stdint.h>

#include "crtfx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crtfx_ingest crtfx_ingest;

/* Plans src_h x src_w -> dst_h x dst_w on `device` and copies the tables (synchronises; the calling thread's current
 * device is restored).  pix_fmt: CRTFX_PIX_U8; CRTFX_PIX_F16 is CRTFX_E_UNSUPPORTED (Pillow has no half image: the
 * reference cannot resize such a frame either).  CRTFX_E_INVALID: a size < 1 or > 32767, a null table, a table that
 * breaks the rules above.  When it fails *out_plan is NULL and crtfx_ingest_last_error(NULL) holds the message
 * (per calling thread). */
int crtfx_ingest_create(int device, int src_h, int src_w, int dst_h, int dst_w, int pix_fmt,
                        const int32_t* x_min, const int32_t* x_count, const int32_t* x_k, int x_ksize,
                        const int32_t* y_min, const int32_t* y_count, const int32_t* y_k, int y_ksize,
                        crtfx_ingest** out_plan);
int crtfx_ingest_destroy(crtfx_ingest* plan);
const char* crtfx_ingest_last_error(const crtfx_ingest* plan);

/* n frames in one call: frame i is read at src_base + i * src_stride_bytes (src_h x src_w x 3 uint8, rows unpadded)
 * and written at dst_base + i * dst_stride_bytes (dst_h x dst_w x 3); strides of at least a frame, any byte alignment.
 * The fused path is one grid for all n frames; the general path runs groups of as many frames as its scratch holds.
 * Bytes between frames are neither read nor written.  Source and destination must not overlap. */
int crtfx_ingest_run(crtfx_ingest* plan, const void* src_base, size_t src_stride_bytes, void* dst_base,
                     size_t dst_stride_bytes, int n, void* stream);

/* Testing / A-B switches of one plan.  FORCE_GENERAL (0 / 1): take k_ingest_h + k_ingest_v whatever the footprint. */
typedef enum crtfx_ingest_option { CRTFX_INGEST_OPT_FORCE_GENERAL = 1 } crtfx_ingest_option;
int crtfx_ingest_set_option(crtfx_ingest* plan, int option, int value);

/* The path of the most recent crtfx_ingest_run (before the first one: the path the next one takes), in the style of
 * crtfx_last_plan: `ingest=k_ingest_fused<rows=32,cols=128>;lds=11880;frames=5` or `ingest=k_ingest_h+k_ingest_v;frames=5`. */
int crtfx_ingest_last_plan(crtfx_ingest* plan, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* CRTFX_INGEST_H */
