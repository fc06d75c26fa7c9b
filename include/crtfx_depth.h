/*
 * crtfx_depth.h — the depth stage of libcrtfx.so: h x w x 3 RGB frames change their sample type on the device.  WIDEN turns uint8 frames
 * (CRTFX_PIX_U8) into half frames (CRTFX_PIX_F16) of the same codes, NARROW turns finished half frames into uint8 ones with a stated
 * rounding, plain or ordered dither.  It stands where a host pipeline has `format=`: behind the 8-bit source stages when the chain runs
 * on half pixels, and in front of the 8-bit egress stages behind such a chain (pythoncrt_amd/depth.py, ends.py), so that the two ends of a
 * render need not have the same depth and an 8-bit job can ask for the half chain.
 *
 * Status codes (crtfx_status) and conventions are those of crtfx.h: the caller owns every frame; work is enqueued on the caller's
 * hipStream_t (void*, NULL = the default stream); only destroy synchronises; the calling thread's current device must be the plan's when
 * it runs.  The stage depends on a device and four numbers, not on a crtfx_ctx: it has a handle of its own, and the handle owns no device
 * memory.
 *
 * Arithmetic, bit for bit (tests/depth_model.py restates it in numpy, tests/test_depth_tables.py and test_depth_gpu.py hold the kernels
 * to it with no differing element).
 * WIDEN:  out = half(u) for u in 0..255.  Exact: every code is a half.
 * NARROW: f = float(half);  v = min(max(f, 0), 255) with NaN -> 0, so -0, negatives and -inf give 0 and +inf gives 255; then
 *     CRTFX_DITHER_NONE:     u = rint_to_even(v) — the rule of the uint8 chain's own convertScaleAbs quantiser and of the 10-bit egress
 *                            quantisers;
 *     CRTFX_DITHER_ORDERED:  u = floor(v + t[y & 7][x & 7]),  t = (2 * B + 1) / 128,  B = CRTFX_DEPTH_BAYER8 below: the 8 x 8 Bayer index
 *                            matrix 0..63 of the usual recursive 2 x 2 construction (M2 = [0 2; 3 1], M2n = [4M 4M+2; 4M+3 4M+1]).
 * (y, x) is the pixel's place in the frame the stage is given; one threshold serves the three channels of a pixel, so grey stays grey.
 * t < 1 and v <= 255, so the result never passes 255.  For every half in [0, 255] and every threshold v + t is exactly representable in
 * float32 (a half in [2^e, 2^(e+1)) ends at bit e - 10, a threshold at bit -7, and the sum spans at most 24 bits; test_depth_tables.py
 * checks all 65 536 x 64 sums against float64), so the floor is the only rounding.  Over an aligned 8 x 8 tile of a constant quarter code
 * q / 4 the mean of the 64 results is exactly q / 4.
 *
 * Frames: 3 bytes per pixel on the uint8 side, 6 on the half side, rows unpadded.  Half-side frame bases and strides must be even
 * (CRTFX_E_INVALID otherwise); uint8 frames may start anywhere.
 *
 * Paths; both give the same bytes, the path is chosen per run, and *_last_plan names the one that ran.
 * k_narrow<dither,vec>: runs where
 *     w % 8 == 0, both frame bases are multiples of 4, and (n > 1) both frame strides are multiples of 4
 * — the rule of crtfx_deep.h.  One lane owns 1 row x 8 pixels: it reads their 48 bytes of halves as three 16-byte loads at a
 * dword-aligned address and writes their 24 bytes as one 16-byte and one 8-byte store at a dword-aligned address; its eight thresholds
 * are row y & 7 of the matrix (one 8-byte load of the index row).  All n frames are one grid (grid.z).
 * k_widen<vec>: the frame's h * w * 3 samples are cut into chunks of 16, one lane per chunk, all n frames in one grid.  It runs where
 *     both frame bases are multiples of 4, (n > 1) both frame strides are multiples of 4, and the frame has fewer than 2^31 samples
 * — nothing is asked of w.  A whole chunk is one 16-byte load at a dword-aligned address and two 16-byte stores at dword-aligned
 * addresses; the frame's last, short chunk is taken by dword (one dword load, eight bytes stored per four samples) and its last one to
 * three samples by byte (a 1-byte load, a 2-byte store each).
 * k_narrow<dither,general>, k_widen<general>: any size and alignment, and the CRTFX_DEPTH_OPT_FORCE_GENERAL fallback: one lane per
 * sample, one 2-byte (1-byte) load and one 1-byte (2-byte) store; grid = (row samples, rows, frames).
 * No element outside a frame is read or written; every destination element is written by exactly one lane on either path; bytes between
 * frames are neither read nor written.
 *
 * Registers (gfx950, as built; tests/test_depth_tables.py reads them from the library and holds every build to 64 VGPRs + AGPRs):
 * k_narrow<none,vec> 24 VGPRs, k_narrow<ordered,vec> 36, k_narrow<none,general> 4, k_narrow<ordered,general> 7, k_widen<vec> 22,
 * k_widen<general> 4 (eight waves per SIMD each); no AGPRs, no LDS, no scratch, no spills.
 *
 * Kernel time per frame, measured once on one MI355X in batches of 8 (tools/depth_kernel_times.py, HIP events; profiles/depth.txt holds the
 * whole output), next to a device-to-device copy of the same traffic (a frame's uint8 bytes + its half bytes) timed in the same run:
 *     1080p   widen  vec  3.1 us  general  7.5    narrow<none>  vec  2.7  general  8.2    narrow<ordered>  vec  2.9  general  8.8    copy  2.3
 *     4K      widen  vec 12.8     general 43.2    narrow<none>  vec 12.4  general 45.2    narrow<ordered>  vec 13.2  general 48.0    copy 13.8
 * vec runs at 0.90 - 0.96 x the copy at 4K and 1.20 - 1.36 x at 1080p; the ordered dither costs 6 - 7 % over plain rounding; general takes
 * 3.1 - 3.9 x the copy and 2.4 - 3.7 x the vec path.  vec is the faster one in every case measured, so it runs whenever its conditions hold.
 */
#ifndef CRTFX_DEPTH_H
#define CRTFX_DEPTH_H

#include <stddef.h>
#include <stdint.h>

#include "crtfx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crtfx_depth crtfx_depth;

typedef enum crtfx_depth_direction { CRTFX_DEPTH_WIDEN = 0, CRTFX_DEPTH_NARROW = 1 } crtfx_depth_direction;
typedef enum crtfx_dither { CRTFX_DITHER_NONE = 0, CRTFX_DITHER_ORDERED = 1 } crtfx_dither;

/* B[y][x], row by row: the threshold of pixel (y, x) is (2 * B[y & 7][x & 7] + 1) / 128 */
#define CRTFX_DEPTH_BAYER8 { \
     0, 32,  8, 40,  2, 34, 10, 42, \
    48, 16, 56, 24, 50, 18, 58, 26, \
    12, 44,  4, 36, 14, 46,  6, 38, \
    60, 28, 52, 20, 62, 30, 54, 22, \
     3, 35, 11, 43,  1, 33,  9, 41, \
    51, 19, 59, 27, 49, 17, 57, 25, \
    15, 47,  7, 39, 13, 45,  5, 37, \
    63, 31, 55, 23, 61, 29, 53, 21 }

/* Plans the conversion of h x w x 3 frames on `device` (the calling thread's current device is restored).  CRTFX_E_INVALID: a null out
 * pointer, an unknown direction or dither, h or w < 1 or > 32767, a dither other than CRTFX_DITHER_NONE with CRTFX_DEPTH_WIDEN (widening
 * is exact: there is nothing to dither).  All of these are refused before a device is touched.  When it fails *out_plan is NULL and
 * crtfx_depth_last_error(NULL) holds the message (per calling thread), which names the offending field. */
int crtfx_depth_create(int device, int h, int w, int direction, int dither, crtfx_depth** out_plan);
int crtfx_depth_destroy(crtfx_depth* plan);
const char* crtfx_depth_last_error(const crtfx_depth* plan);

/* n frames in one call: frame i is read at src_base + i * src_stride_bytes and written at dst_base + i * dst_stride_bytes (h x w x 3
 * samples each, rows unpadded; WIDEN reads uint8 and writes half, NARROW the reverse).  n = 0 does nothing.  CRTFX_E_INVALID: n < 0, a
 * null frame pointer, a stride shorter than a frame (n > 1), an odd base or stride on the half side, and a source range [src_base,
 * src_base + (n - 1) * stride + frame) that overlaps the destination's.  Bytes between frames are neither read nor written. */
int crtfx_depth_run(crtfx_depth* plan, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n,
                    void* stream);

/* Testing / A-B switches of one plan.  FORCE_GENERAL (0 / 1): take the general kernel whatever the width and alignment. */
typedef enum crtfx_depth_option { CRTFX_DEPTH_OPT_FORCE_GENERAL = 1 } crtfx_depth_option;
int crtfx_depth_set_option(crtfx_depth* plan, int option, int value);

/* The path of the most recent crtfx_depth_run (before the first one: the path a run with aligned frames takes):
 * `depth=k_narrow<ordered,vec>;frames=5`, `depth=k_narrow<none,general>;frames=5`, `depth=k_widen<vec>;frames=5` or
 * `depth=k_widen<general>;frames=5`. */
int crtfx_depth_last_plan(crtfx_depth* plan, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* CRTFX_DEPTH_H */
