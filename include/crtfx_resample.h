/*
 * crtfx_resample.h — the filtered resampler of libcrtfx.so: h x w x 3 RGB frames, uint8 (CRTFX_PIX_U8) or half on the 0..255 scale
 * (CRTFX_PIX_F16), of one size resized on the device to another with any of Pillow's five 8-bit resampling filters — BOX, BILINEAR, HAMMING,
 * BICUBIC, LANCZOS — uint8 frames byte for byte as `Image.resize((w, h), filter)` does it.  It stands beside crtfx_ingest_* (crtfx_ingest.h)
 * and crtfx_resize16_* (crtfx_resize16.h), which are BILINEAR only and stay as they are: their tables are non-negative and their
 * accumulators unsigned, and bicubic and Lanczos have negative lobes, three times the taps, and results that overshoot at both ends.
 *
 * Status codes (crtfx_status), pixel formats (crtfx_pixfmt) and conventions are those of crtfx.h: the caller owns every frame; work is
 * enqueued on the caller's hipStream_t (void*, NULL = the default stream); only create / destroy synchronise; the calling thread's current
 * device must be the plan's when it runs.  The stage depends on a device, two sizes, a pixel format and two coefficient tables, not on a
 * crtfx_ctx: it has a handle of its own.
 *
 * Arithmetic (Pillow's 8-bit resampler, src/libImaging/Resample.c).  The tables are HOST arrays built with Pillow's float64 expressions
 * (pythoncrt_amd.tables.pil_filter_axis) and copied by crtfx_resample_create: per output index the first tap `min`, the tap count `count`
 * and `ksize` SIGNED coefficients.  A pass along one axis computes
 *     out[xx] = clamp((2^21 + sum_{t < count[xx]} k[xx][t] * in[xmin[xx] + t]) >> 22, 0, top)          the shift arithmetic, the sum signed
 * The horizontal pass runs first, its result is rounded and clamped, and the vertical pass reads that (the two passes cannot be contracted
 * into one 2-D sum).  An axis whose size does not change has identity tables under all five filters (one tap of 2^22: Pillow skips that
 * pass, and running it gives the same samples), so both passes always run.
 *   CRTFX_PIX_U8   top = 255; the samples are the bytes.  A tap is one signed 24-bit multiply-add into an int32.
 *   CRTFX_PIX_F16  top = 1020, on the quarter-code scale of crtfx_resize16.h:
 *                  in:  q = rint_to_even(min(max(4 * float(half), 0), 1020)), NaN -> 0   (-0, negatives, -inf -> 0; +inf -> 1020)
 *                  both passes on quarter codes; out: half(q / 4), exact.
 *                  The sum of a row no longer fits 32 bits, signed or unsigned (Lanczos at 2:1: positive taps of 1.27 x 2^22, times 1020 =
 *                  5.4e9).  It is held in two int32 accumulators, A = sum k * (q >> 2) and B = sum k * (q & 3), one signed 24-bit
 *                  multiply-add each per tap, and combined once per sample as (2^21 + 4 A + B) >> 22 in 64 bits: exactly the int64 sum.
 *                  CRTFX_RESAMPLE_OPT_ACC64 takes a 64-bit multiply-add per tap instead (an A/B switch: the same bits).
 *
 * Table rules (CRTFX_E_INVALID otherwise; checked on the host before a device is touched):
 *     1 <= count <= ksize, min >= 0, min + count <= n_in; min and min + count non-decreasing          (the window rules of crtfx_ingest.h)
 *     -2^23 <= k < 2^23                                                                                 (a signed 24-bit operand)
 *     per row: 2^21 + 255 * (sum of the positive k) < 2^31 and 255 * (sum of the negative k) > -2^31
 * The last rule bounds every partial sum of a uint8 pass inside int32, and for half frames those of A (q >> 2 <= 255) and of B (q & 3 <= 3).
 * Pillow's tables meet it with room: the positive taps of a row sum to at most 1.125 x 2^22 (bicubic) and 1.272 x 2^22 (Lanczos).
 *
 * Frames: rows unpadded, 3 or 6 bytes per pixel.  Half frames: every frame base and frame stride must be even (CRTFX_E_INVALID otherwise).
 *
 * Paths; both give the same bits, and *_last_plan names the one that ran.
 * k_resample_fused<u8|half>: one block of 256 threads per tile of output rows x output columns.  The source rows and columns the tile's
 * taps reach are staged into LDS as aligned dwords (a row keeps its global address modulo 4; a dword that sticks out of the frame's own
 * bytes is assembled from byte loads, so nothing outside a frame is read), halves quantised to uint16 quarter codes on the way; the
 * horizontal pass runs LDS to LDS; the vertical pass reads its result and stores aligned dwords of four bytes / two halves (the samples in
 * front of and behind the aligned dwords of the tile's row segment are single items).  Every output element is written by exactly one
 * lane.  It serves every size pair for which some tile shape of
 *     (rows, columns) in (32,128) (32,64) (16,128) (16,64) (8,64) (8,32) (4,32)        — the first that fits is taken —
 * has a footprint of at most 40 960 bytes of LDS (four blocks per CU), where, over all tiles of that shape and with b = 1 or 2 bytes a sample,
 *     footprint = 4 * (2 * cols + cols * x_ksize + 2 * rows + rows * y_ksize)                            the tile's tables
 *               + max_source_rows * (round4(3 b * max_source_cols + 3) + round4(3 b * cols) + 4)         staged source + horizontal result
 * (cols / rows clipped to the output size): the rule of crtfx_ingest.h.  Lanczos 4K -> 1080p and 8K -> 4K take (16,64) at 30 672 bytes on
 * uint8 and (8,64) at 36 040 on halves; 1080p -> 4K takes (32,128) at 19 048 / 32 072; bicubic 4K -> 1080p (16,64) at 26 472 and (8,64) at
 * 29 480; Lanczos 4K -> 960 x 540 fits (8,32) on uint8 and no shape on halves.  Everything else, and everything under FORCE_GENERAL, takes
 * the general path: k_resample_h<u8|half> writes the horizontal pass to a src_h x dst_w x 3 scratch of samples the plan owns (as many frames
 * as fit 64 MiB, at least one, at most 64; behind a fused plan, where the general path is an A/B switch only, one), k_resample_v<u8|half>
 * runs the vertical pass over it.  The general path quantises a half source sample once per tap that reads it.
 *
 * Registers (gfx950, as built; tests/test_resample_tables.py reads them from the library and holds every build to these numbers):
 *     k_resample_fused  u8 43   half 56   half/acc64 43
 *     k_resample_h      u8 29   half 40   half/acc64 18
 *     k_resample_v      u8 6    half 8    half/acc64 7
 * VGPRs (at most 64: eight waves per SIMD each); no AGPRs, no static LDS (the fused kernel's block is dynamic: its size is the plan's `lds`), no scratch, no spills.
 */
#ifndef CRTFX_RESAMPLE_H
#define CRTFX_RESAMPLE_H

#include <stddef.h>
#include <stdint.h>

#include "crtfx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crtfx_resample crtfx_resample;

/* Plans src_h x src_w -> dst_h x dst_w on `device` and copies the tables (synchronises; the calling thread's current device is restored).
 * pix_fmt: CRTFX_PIX_U8 or CRTFX_PIX_F16.  CRTFX_E_INVALID: another pixel format, a size < 1 or > 32767, a null table, a table that breaks
 * the rules above.  All of these are refused before a device is touched.  When it fails *out_plan is NULL and crtfx_resample_last_error(NULL)
 * holds the message (per calling thread). */
int crtfx_resample_create(int device, int src_h, int src_w, int dst_h, int dst_w, int pix_fmt,
                          const int32_t* x_min, const int32_t* x_count, const int32_t* x_k, int x_ksize,
                          const int32_t* y_min, const int32_t* y_count, const int32_t* y_k, int y_ksize,
                          crtfx_resample** out_plan);
int crtfx_resample_destroy(crtfx_resample* plan);
const char* crtfx_resample_last_error(const crtfx_resample* plan);

/* n frames in one call: frame i is read at src_base + i * src_stride_bytes (src_h x src_w x 3 samples, rows unpadded) and written at
 * dst_base + i * dst_stride_bytes (dst_h x dst_w x 3 samples); strides of at least a frame; uint8 frames at any byte alignment, half frames
 * with even bases and strides.  The fused path is one grid for all n frames; the general path runs groups of as many frames as its scratch
 * holds.  Bytes between frames are neither read nor written.  Source and destination must not overlap. */
int crtfx_resample_run(crtfx_resample* plan, const void* src_base, size_t src_stride_bytes, void* dst_base,
                       size_t dst_stride_bytes, int n, void* stream);

/* Testing / A-B switches of one plan.  FORCE_GENERAL (0 / 1): take k_resample_h + k_resample_v whatever the footprint.
 * ACC64 (0 / 1; half frames only, CRTFX_E_INVALID on a uint8 plan): a 64-bit multiply-add per tap in place of the two int32 accumulators. */
typedef enum crtfx_resample_option { CRTFX_RESAMPLE_OPT_FORCE_GENERAL = 1, CRTFX_RESAMPLE_OPT_ACC64 = 2 } crtfx_resample_option;
int crtfx_resample_set_option(crtfx_resample* plan, int option, int value);

/* The path of the most recent crtfx_resample_run (before the first one: the path the next one takes):
 * `resample=k_resample_fused<u8,rows=16,cols=64>;lds=30672;frames=5` or `resample=k_resample_h+k_resample_v<half>;frames=5`
 * (`;acc=i64` behind it under ACC64). */
int crtfx_resample_last_plan(crtfx_resample* plan, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* CRTFX_RESAMPLE_H */
