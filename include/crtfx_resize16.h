/*
 * crtfx_resize16.h — the half resampler of libcrtfx.so: h x w x 3 half RGB frames (CRTFX_PIX_F16, IEEE half on the 0..255 scale) of one
 * size resized on the device to another.  It stands behind a chain that runs on half pixels, where crtfx_ingest_* (crtfx_ingest.h) stands
 * for uint8 frames: a 10-bit render at one size is delivered at another without a host core touching a sample.
 *
 * Status codes (crtfx_status), pixel formats (crtfx_pixfmt) and conventions are those of crtfx.h: the caller owns every frame; work is
 * enqueued on the caller's hipStream_t (void*, NULL = the default stream); only create / destroy synchronise; the calling thread's current
 * device must be the plan's when it runs.  The stage depends on a device, two sizes and two coefficient tables, not on a crtfx_ctx: it has
 * a handle of its own.
 *
 * Arithmetic: Pillow's 8-bit two-pass BILINEAR resampler (crtfx_ingest.h) on the 10-bit "quarter code" scale of crtfx_deep.h, q = 0..1020
 * for the half value q / 4.  With the tables of pythoncrt_amd.tables.pil_resample_axis — the ones crtfx_ingest_create takes, under the
 * same rules — and unsigned 32-bit accumulators:
 *     in:   q = rint_to_even(min(max(4 * float(half), 0), 1020)), NaN -> 0         (crtfx_egress10's quantiser: -0, negatives, -inf -> 0; +inf -> 1020)
 *     pass: out[xx] = min((2^21 + sum_{t < count[xx]} k[xx][t] * in[xmin[xx] + t]) >> 22, 1020)
 *           horizontal first, its result a quarter code (uint16); the vertical pass reads that (the two passes cannot be contracted)
 *     out:  half(q / 4)                                                             exact: every quarter code is a half, no rounding occurs
 * The half -> float conversion and 4 f are exact; the roundings are the rint and the >> 22 of each pass.  create refuses a table with a row
 * for which sum_{t < count} k * 1020 + 2^21 >= 2^32, so no accumulator wraps; the rows of pil_resample_axis sum to 2^22 within a few units
 * (each tap rounds once: 2^22 - 2 .. 2^22 + 3 over every size pair tried, 4K <-> 1080p, 8K -> 1080p and 32767 -> 1 among them, so the
 * largest accumulator is 4 280 290 292 of 4 294 967 295), and no real table is
 * refused.  With k < 2^24 and q <= 1020 both factors fit 24 bits: a tap is one 24-bit multiply-add.
 *
 * Frames: rows unpadded, 6 bytes per pixel.  Every frame base and frame stride must be even (CRTFX_E_INVALID otherwise).
 *
 * Paths; both give the same bits, and *_last_plan names the one that ran.
 * k_resize16_fused: one block per tile of output rows x output columns.  The source rows and columns the tile's taps reach are quantised
 * once while they are staged into LDS as uint16 (aligned dwords: a row keeps its global address modulo 4; a dword that sticks out of the
 * frame's own bytes is assembled from 16-bit loads, so nothing outside a frame is read); the horizontal pass writes uint16 to LDS; the
 * vertical pass reads it and stores aligned dwords of two halves (a single half in front of and behind them where the tile's row segment
 * starts or ends off a dword).  Every output element is written by exactly one lane.  It serves every size pair for which some tile shape of
 *     (rows, columns) in (32,128) (32,64) (16,128) (16,64) (8,64) (8,32) (4,32)        — the first that fits is taken —
 * has a footprint of at most 40 960 bytes of LDS (four blocks per CU), where, over all tiles of that shape,
 *     footprint = 4 * (2 * cols + cols * x_ksize + 2 * rows + rows * y_ksize)                      the tile's tables
 *               + max_source_rows * (round4(6 * max_source_cols + 2) + round4(6 * cols))           staged source + horizontal result
 * (cols / rows clipped to the output size): the rule of crtfx_ingest.h with 2-byte samples.  That holds for every up-scale ((32,128) at
 * 2x: 18 source rows x (400 + 768) bytes + 3 200 of tables = 24 224), for 1/2 on both axes ((8,64): 4K -> 1080p is 18 x (784 + 384) + 2 016
 * = 23 040) and for every ratio down to 1/4 on both axes ((8,32): 4K -> 540p is 36 x (796 + 192) + 1 760 = 37 328; (4,32) where a tile's
 * window is a row or two longer), and for stronger reductions of small images.  Everything else — the tap count grows with the down-scale
 * factor without bound — takes the general path: k_resize16_h writes the horizontal pass to a uint16 src_h x dst_w x 3 scratch the plan
 * owns (as many frames as fit 64 MiB, at least one, at most 64; behind a fused plan, where the general path is an A/B switch only, one),
 * k_resize16_v runs the vertical pass over it.  The general path quantises a source sample once per tap that reads it.
 *
 * Registers (gfx950, as built; tests/test_resize16_tables.py reads them from the library and holds every build to 128):
 * k_resize16_fused 43 VGPRs, k_resize16_h 32, k_resize16_v 6 (eight waves per SIMD each); no AGPRs, no static LDS (the fused kernel's block is dynamic: its
 * size is the plan's `lds`), no scratch, no spills.
 */
#ifndef CRTFX_RESIZE16_H
#define CRTFX_RESIZE16_H

#include <stddef.h>
#include <stdint.h>

#include "crtfx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crtfx_resize16 crtfx_resize16;

/* Plans src_h x src_w -> dst_h x dst_w on `device` and copies the tables (synchronises; the calling thread's current device is restored).
 * pix_fmt: CRTFX_PIX_F16; CRTFX_PIX_U8 is CRTFX_E_UNSUPPORTED (only half frames are resized here: uint8 frames have crtfx_ingest_*).
 * CRTFX_E_INVALID: a size < 1 or > 32767, a null table, a table that breaks the rules of crtfx_ingest.h, a row whose accumulator could
 * wrap (above).  All of these are refused before a device is touched.  When it fails *out_plan is NULL and
 * crtfx_resize16_last_error(NULL) holds the message (per calling thread). */
int crtfx_resize16_create(int device, int src_h, int src_w, int dst_h, int dst_w, int pix_fmt,
                          const int32_t* x_min, const int32_t* x_count, const int32_t* x_k, int x_ksize,
                          const int32_t* y_min, const int32_t* y_count, const int32_t* y_k, int y_ksize,
                          crtfx_resize16** out_plan);
int crtfx_resize16_destroy(crtfx_resize16* plan);
const char* crtfx_resize16_last_error(const crtfx_resize16* plan);

/* n frames in one call: frame i is read at src_base + i * src_stride_bytes (src_h x src_w x 3 halves, rows unpadded) and written at
 * dst_base + i * dst_stride_bytes (dst_h x dst_w x 3 halves); strides of at least a frame; bases and strides even.  The fused path is one
 * grid for all n frames; the general path runs groups of as many frames as its scratch holds.  Bytes between frames are neither read nor
 * written.  Source and destination must not overlap. */
int crtfx_resize16_run(crtfx_resize16* plan, const void* src_base, size_t src_stride_bytes, void* dst_base,
                       size_t dst_stride_bytes, int n, void* stream);

/* Testing / A-B switches of one plan.  FORCE_GENERAL (0 / 1): take k_resize16_h + k_resize16_v whatever the footprint. */
typedef enum crtfx_resize16_option { CRTFX_RESIZE16_OPT_FORCE_GENERAL = 1 } crtfx_resize16_option;
int crtfx_resize16_set_option(crtfx_resize16* plan, int option, int value);

/* The path of the most recent crtfx_resize16_run (before the first one: the path the next one takes):
 * `resize16=k_resize16_fused<rows=32,cols=128>;lds=24224;frames=5` or `resize16=k_resize16_h+k_resize16_v;frames=5`. */
int crtfx_resize16_last_plan(crtfx_resize16* plan, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* CRTFX_RESIZE16_H */
