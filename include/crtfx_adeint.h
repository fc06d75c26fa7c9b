/*
 * crtfx_adeint.h — the motion-adaptive deinterlace stage of libcrtfx.so: an h x w x 3 RGB frame (CRTFX_PIX_U8 or CRTFX_PIX_F16) that carries
 * two fields woven into its even and odd rows becomes one progressive frame or two, as in crtfx_deint.h, but the rows a field lacks are
 * taken from the OTHER field where the picture did not change since the previous frame (the weave: full vertical resolution, no bob) and
 * from CRTFX_DEINT_EDGE's interpolation where it did.  It stands where the Deinterlace stands (pythoncrt_amd/adeint.py, ends.py).  It is
 * causal: it needs the previous source frame only — no lookahead, no latency, the frame count of crtfx_deint.h.
 *
 * Status codes, pixel formats and conventions are those of crtfx.h and crtfx_deint.h: the caller owns every frame, the previous one
 * included; work is enqueued on the caller's hipStream_t; only destroy synchronises; the calling thread's current device must be the
 * plan's when it runs.  The handle owns no device memory and keeps nothing from one run to the next: the previous frame of a run's first
 * frame is an argument of that run.
 *
 * Arithmetic, bit for bit; this is the library's own rule (tests/adeint_model.py restates it in numpy, tests/test_adeint_tables.py and
 * test_adeint_gpu.py hold the kernels to it with no differing element).  NOT claimed is equality with any other deinterlacer, yadif and
 * bwdif included.
 * Shared with crtfx_deint.h, exactly: the inputs, the sample types and the quarter-code quantiser of half frames, CRTFX_DEINT_TFF / BFF,
 * CRTFX_DEINT_FIRST / BOTH and BOTH's frame numbering, and kept rows (y % 2 == F) copied as bits.
 * The previous frame P.  Each source frame C has a previous frame P: within a batch the frame before C; for frame 0 of a run the caller's
 * prev_frame, or none (NULL).
 * Made rows.  For an output frame made for field F a made row is a row y with y % 2 != F.  With c[.] and p[.] the codes of C and P, and
 * e[x][k] what CRTFX_DEINT_EDGE writes at that sample (the same search, the same d = 0 columns, a row with one neighbour a copy of it):
 *     no P:                 out[x][k] = e[x][k]                      (the frame is exactly EDGE's)
 *     with P, per pixel x:  t0 = max over k of |c[y][x][k] - p[y][x][k]|
 *                           t1 = max over k of (|c[y-1][x][k] - p[y-1][x][k]| + |c[y+1][x][k] - p[y+1][x][k]| + 1) >> 1
 *                                (one neighbour row r in the frame: t1 = max over k of |c[r][x][k] - p[r][x][k]|)
 *                           m  = max(t0, t1)
 *                           out[x][k] = min(max(e[x][k], c[y][x][k] - m), c[y][x][k] + m)
 * One m is shared by a pixel's three channels, so that grey stays grey; EDGE's direction follows the same convention.  The result lies
 * between e and c[y], both codes, so no clamp to the code range is needed.  It is written as the family writes: the code itself for
 * uint8, half(r / 4) for half.
 * What follows: where P equals C in the three rows, m = 0 and the made sample is C's own row y — the weave; for uint8 the whole output
 * frame is then the source frame, for either field.  Where m >= |e - c[y]| the sample is EDGE's.  BOTH is FIRST of the two orders
 * interleaved.  Each output frame depends on source frames i - 1 and i only.
 * Why one frame pair serves both fields: row y of C is the neighbouring field in time — one field later for the first field's frame, one
 * field earlier for the second's.  |C - P| on row y compares that field with its own previous instance; |C - P| on rows y +- 1 compares
 * the kept field with its previous instance.
 *
 * Frames: as in crtfx_deint.h (3 or 6 bytes per pixel, rows unpadded, n counts SOURCE frames, the destination stride is per OUTPUT frame,
 * half frames need even bases and strides).  prev_frame is one frame of h x w x 3 samples.
 *
 * Paths; both give the same bytes, the path is chosen per run, and *_last_plan names the one that ran.
 * k_adeint<pix,fields,vec>: runs where k_deint<...,vec> runs — w % 8 == 0, both frame bases multiples of 4, the source stride a multiple
 *     of 4 (n > 1) and the destination's (more than one OUTPUT frame) — and prev_frame, when it is not NULL, is a multiple of 4.  One lane
 *     owns 1 row x 8 pixels of the SOURCE frame and that block of every output frame; all n source frames are one grid (grid.z).  Every
 *     load is a dword-multiple access at a dword-aligned address.  A lane always loads its block of C's row y (the kept bits, and the centre
 *     of the clamp).  Where the block is made it loads what k_deint<edge,...,vec> loads — its block of rows y - 1 and y + 1 and the four
 *     pixels on either side where the row has them — and its own block of P's rows y - 1, y, y + 1: no halo there, m is per pixel.  Under
 *     BOTH a lane does both, the kept block into one output frame and the made block into the other: one launch writes both frames.
 * k_adeint<pix,fields,general>: any size and alignment, and the CRTFX_ADEINT_OPT_FORCE_GENERAL fallback: one lane per pixel of the source
 *     frame, which owns that pixel of every output frame; 1-byte (2-byte) loads and stores; grid = (pixels of a row, rows, frames).
 * Every output element is written by exactly one lane on either path; nothing outside a source frame, P or an output frame is read or
 * written.  A launch covers at most 32 768 source frames; the first frame of a later launch takes the last frame of the launch before it
 * as P.
 * The direction search, the sample types and the dword helpers are SHARED with crtfx_deint.hip (csrc/crtfx_edge.hip.h), not restated: the
 * sixteen k_deint builds keep the registers crtfx_deint.h quotes.
 *
 * Registers (gfx950, as built; tests/test_adeint_tables.py reads them from the library): VGPRs of k_adeint<pix,fields,path>
 *     k_adeint<u8,first,vec> 126, k_adeint<u8,both,vec> 128, k_adeint<f16,first,vec> 148, k_adeint<f16,both,vec> 150,
 *     k_adeint<u8,first,general> 63, k_adeint<u8,both,general> 63, k_adeint<f16,first,general> 66, k_adeint<f16,both,general> 64
 * (four waves per SIMD for the uint8 vec builds, three for the half ones, seven or eight for the general builds: beside EDGE's 2 x 14 x 3
 * codes a lane holds the 24 codes of its own block and eight m); no AGPRs, no LDS, no scratch, no spills.
 *
 * Kernel time per SOURCE frame, measured once on one MI355X in batches of 8 in which every frame has a previous frame and half the rows of
 * every frame are those of the frame before it (tools/adeint_kernel_times.py, HIP events; profiles/adeint.txt holds the whole output),
 * next to two yardsticks timed in the same run: the untouched k_deint<edge,...> build of the same path, and a device-to-device copy of equal
 * traffic (each source frame read once + the output frames written); us, vec / general / EDGE vec / EDGE general / copy:
 *                          uint8                                half
 *     480 x 720    first    2.3 /  5.5 / 1.7 /  4.4 / 0.4        3.8 /  5.6 /  2.5 /  4.5 / 0.5
 *                  both     2.4 /  7.8 / 1.9 /  6.7 / 0.4        4.0 /  8.0 /  2.9 /  6.8 / 0.9
 *     1080 x 1920  first    7.9 / 44.9 / 6.1 / 34.1 / 1.6       13.7 / 45.3 /  8.9 / 34.4 / 3.5
 *                  both    11.0 / 47.0 / 8.0 / 39.6 / 2.3       18.8 / 47.9 / 11.9 / 40.3 / 6.8
 * Eight frames of either size lie in the Infinity Cache, so the copy runs above the HBM rate and is a hard yardstick.  The vec path takes
 * 1.29 - 1.38 x EDGE's vec path on uint8 frames and 1.38 - 1.58 x on half frames (four more blocks loaded and, of halves, 96 more samples
 * quantised per lane — two at a time, in packed half arithmetic: P::codes of crtfx_edge.hip.h), 4.8 - 5.6 x the
 * copy on uint8 frames and 2.8 - 7.4 x on half frames; like EDGE it is bound by its arithmetic, not by memory.  The general path takes
 * 1.17 - 1.32 x EDGE's general path.  vec takes 0.18 - 0.67 x the general path: it is the faster path in every case measured, so it runs
 * whenever its conditions hold.
 */
#ifndef CRTFX_ADEINT_H
#define CRTFX_ADEINT_H

#include <stddef.h>
#include <stdint.h>

#include "crtfx.h"
#include "crtfx_deint.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crtfx_adeint crtfx_adeint;

/* Plans the motion-adaptive deinterlacing of h x w x 3 frames of pix_fmt (CRTFX_PIX_U8 or CRTFX_PIX_F16) on `device` (the calling thread's
 * current device is restored); order is a crtfx_deint_order, fields a crtfx_deint_fields.  CRTFX_E_INVALID: what crtfx_deint_create
 * refuses — a null out pointer, h < 2 or > 32767, w < 1 or > 32767, an unknown pix_fmt, order or fields — before a device is touched.
 * When it fails *out_plan is NULL and crtfx_adeint_last_error(NULL) holds the message (per calling thread), which names the field. */
int crtfx_adeint_create(int device, int h, int w, int pix_fmt, int order, int fields, crtfx_adeint** out_plan);
int crtfx_adeint_destroy(crtfx_adeint* plan);
const char* crtfx_adeint_last_error(const crtfx_adeint* plan);

/* Output frames per source frame: 1 (FIRST) or 2 (BOTH); 0 for a null plan. */
int crtfx_adeint_frames_out(const crtfx_adeint* plan);

/* n SOURCE frames in one call, laid out as crtfx_deint_run's.  prev_frame is the frame in front of source frame 0, or NULL: frame 0 then
 * has no previous frame and its output is EDGE's.  n = 0 does nothing.  CRTFX_E_INVALID: every refusal of crtfx_deint_run, an odd
 * prev_frame for half frames, and a prev_frame range [prev_frame, prev_frame + frame) that overlaps the destination's.  prev_frame may
 * lie anywhere else, inside the source range included. */
int crtfx_adeint_run(crtfx_adeint* plan, const void* prev_frame, const void* src_base, size_t src_stride_bytes, void* dst_base,
                     size_t dst_stride_bytes, int n, void* stream);

/* Testing / A-B switches of one plan.  FORCE_GENERAL (0 / 1): take the general kernel whatever the width and alignment. */
typedef enum crtfx_adeint_option { CRTFX_ADEINT_OPT_FORCE_GENERAL = 1 } crtfx_adeint_option;
int crtfx_adeint_set_option(crtfx_adeint* plan, int option, int value);

/* The path of the most recent crtfx_adeint_run (before the first one: the path a run with aligned frames takes), frames = the SOURCE
 * frames of that run: `adeint=k_adeint<u8,both,vec>;frames=5`. */
int crtfx_adeint_last_plan(crtfx_adeint* plan, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* CRTFX_ADEINT_H */
