/*
 * crtfx_deint.h — the deinterlace stage of libcrtfx.so: an h x w x 3 RGB frame (CRTFX_PIX_U8 or CRTFX_PIX_F16) that carries two fields
 * woven into its even and odd rows becomes one progressive frame (the first field, its missing rows interpolated) or two (one per field,
 * in field order) on the device.  It stands where a host pipeline has `yadif` or `bwdif` in front of everything else: directly behind the
 * source plan, at the source size, in front of the crop and the resize, which would mix the fields (pythoncrt_amd/deint.py, ends.py).  With
 * both fields sent the chain runs at field rate, and its persistence blend decays field to field as phosphor does.
 *
 * Status codes (crtfx_status), pixel formats (crtfx_pixfmt) and conventions are those of crtfx.h: the caller owns every frame; work is
 * enqueued on the caller's hipStream_t (void*, NULL = the default stream); only destroy synchronises; the calling thread's current device
 * must be the plan's when it runs.  The stage depends on a device and six numbers, not on a crtfx_ctx: it has a handle of its own, the
 * handle owns no device memory, and it keeps nothing from one run to the next (every output frame is a function of one source frame).
 *
 * Arithmetic, bit for bit; this is the library's own rule (tests/deint_model.py restates it in numpy, tests/test_deint_tables.py and
 * test_deint_gpu.py hold the kernels to it with no differing element).  NOT claimed is equality with any other deinterlacer.
 * An output frame is made for a field F (0 = the even rows, 1 = the odd rows).  The first field is 0 under CRTFX_DEINT_TFF and 1 under
 * CRTFX_DEINT_BFF.  CRTFX_DEINT_FIRST writes, per source frame, the frame of the first field; CRTFX_DEINT_BOTH the frame of the first field
 * and then the frame of the other one.
 * Rows with y % 2 == F are copied as bits: every half pattern survives, NaN payloads included (as in crtfx_canvas.h).
 * Every other row is interpolated from the kept rows a = row y - 1 and b = row y + 1, in integers: on the codes 0..255 of uint8 frames; of
 * half frames on quarter codes q = rint_to_even(min(max(4 f, 0), 1020)), NaN -> 0 (the quantiser of crtfx_resize16.h), and the result r is
 * written as half(r / 4), which is exact (every quarter code is a half).  Where only one of a, b lies in the frame (y = 0, or y = h - 1) the
 * row is a copy of that one: its code for uint8, half(q / 4) of its quarter code for half.  Otherwise
 *     CRTFX_DEINT_LINEAR:  out[x][k] = (a[x][k] + b[x][k] + 1) >> 1
 *     CRTFX_DEINT_EDGE:    one direction d per PIXEL, shared by its three channels, so that grey stays grey (the ordered dither of
 *                          crtfx_depth.h has the same rule).  With
 *                              S(j) = sum over t in {-1, 0, 1} and k in {R, G, B} of |a[x + t + j][k] - b[x + t - j][k]|
 *                          the search is
 *                              s = S(0) - 1;  d = 0
 *                              for j in (-1, +1), in this order:
 *                                  if S(j) < s:  s = S(j);  d = j
 *                                      if S(2j) < s:  s = S(2j);  d = 2j     (the second step is tried only behind a successful first one)
 *                              out[x][k] = (a[x + d][k] + b[x - d][k] + 1) >> 1
 *                          A column with x < 3 or x > w - 4 takes d = 0, because the search reaches x +- 3; so does a row with one
 *                          neighbour.  Where d = 0 the result is LINEAR's.  The largest accumulator is 9 * 1020.
 * No clamp is needed: (a + b + 1) >> 1 <= max(a, b), so the mean of two codes of 0..255 (0..1020) is such a code.
 *
 * Frames: 3 bytes per pixel (uint8) or 6 (half), rows unpadded; the same sample type goes in and out.  n counts SOURCE frames and the
 * stage writes n * frames_out frames: source frame i gives output frame i (FIRST) or output frames 2 i and 2 i + 1 (BOTH); the
 * destination stride is per OUTPUT frame.  For half frames every frame base and frame stride must be even (CRTFX_E_INVALID otherwise);
 * uint8 frames may start anywhere.
 *
 * Paths; both give the same bytes, the path is chosen per run, and *_last_plan names the one that ran.
 * k_deint<method,pix,fields,vec>: runs where
 *     w % 8 == 0, both frame bases are multiples of 4, the source stride is a multiple of 4 (n > 1) and so is the destination's (more
 *     than one OUTPUT frame: n > 1, or BOTH)
 * — the rule of crtfx_deep.h.  One lane owns 1 row x 8 pixels of the SOURCE frame, row y and columns 8 c .. 8 c + 7, and with them that
 * block of every output frame; all n source frames are one grid (grid.z).  Where the block is kept (y % 2 == F) the lane reads its 24
 * samples as dword-multiple loads at a dword-aligned address (24 bytes: 16 + 8; 48 bytes of halves: 3 x 16) and stores those bits; where
 * it is made the lane reads the same block of rows y - 1 and y + 1 and stores 24 results the same way.  Under BOTH a lane does both, the
 * kept block into one output frame and the made block into the other: one launch writes the two frames from one pass over the source
 * (a row is read by the lanes of three rows, once from memory and twice from the caches).
 * EDGE reaches three columns past the block on either side.  The lane loads the four pixels on either side of its block, which are 12
 * bytes (24 of halves) at a dword-aligned address — dword-multiple loads again — and half of the neighbouring block OF THE SAME ROW.  A
 * block at a row's end has no neighbour on that side and loads nothing there: its outermost three columns are x < 3 or x > w - 4 and
 * take d = 0 by the rule above, not by a clamped read, and its other five columns reach at most the block's own edge.  So every load is
 * the block of a row of the frame or part of a block beside it in that row, and no element outside a source frame is read.
 * k_deint<method,pix,fields,general>: any size and alignment, and the CRTFX_DEINT_OPT_FORCE_GENERAL fallback: one lane per pixel of the
 * source frame, which owns that pixel of every output frame; 1-byte (2-byte) loads and stores; EDGE loads columns x - 3 .. x + 3 of the two
 * rows only where 3 <= x <= w - 4; grid = (pixels of a row, rows, frames).
 * Every output element is written by exactly one lane on either path; bytes between frames are neither read nor written.
 *
 * Registers (gfx950, as built; tests/test_deint_tables.py reads them from the library): VGPRs of k_deint<method,pix,fields,path>
 *     k_deint<linear,u8,first,vec> 18, k_deint<linear,u8,both,vec> 22, k_deint<linear,f16,first,vec> 31, k_deint<linear,f16,both,vec> 32,
 *     k_deint<edge,u8,first,vec> 89, k_deint<edge,u8,both,vec> 91, k_deint<edge,f16,first,vec> 127, k_deint<edge,f16,both,vec> 129,
 *     k_deint<linear,u8,first,general> 10, k_deint<linear,u8,both,general> 9, k_deint<linear,f16,first,general> 11, k_deint<linear,f16,both,general> 9,
 *     k_deint<edge,u8,first,general> 59, k_deint<edge,u8,both,general> 59, k_deint<edge,f16,first,general> 60, k_deint<edge,f16,both,general> 60
 * (eight waves per SIMD for the LINEAR and the general builds, five for <edge,u8,.,vec>, four and three for <edge,f16,first,vec> and
 * <edge,f16,both,vec>: a lane holds the 2 x 14 x 3 codes its eight searches read); no AGPRs, no LDS, no scratch, no spills.
 *
 * Kernel time per SOURCE frame, measured once on one MI355X in batches of 8 (tools/deint_kernel_times.py, HIP events; profiles/deint.txt
 * holds the whole output), next to a device-to-device copy of equal traffic (one source frame read + the output frames written) timed in
 * the same run; us, vec / general / copy:
 *                                   uint8                   half
 *     480 x 720    linear  first    1.3 /  1.5 / 0.4        1.3 /  1.6 / 0.5
 *                  linear  both     1.3 /  2.6 / 0.5        1.7 /  2.7 / 0.9
 *                  edge    first    1.8 /  4.4 / 0.5        2.5 /  4.5 / 0.5
 *                  edge    both     1.8 /  6.7 / 0.5        2.9 /  6.8 / 0.9
 *     1080 x 1920  linear  first    2.3 /  8.5 / 1.6        4.8 /  8.8 / 3.0
 *                  linear  both     4.4 / 14.2 / 2.3        8.8 / 15.7 / 6.7
 *                  edge    first    6.1 / 34.1 / 1.8        8.9 / 34.3 / 3.5
 *                  edge    both     8.1 / 39.6 / 2.3       12.1 / 40.3 / 6.7
 * Eight frames of either size lie in the Infinity Cache, so the copy runs above the HBM rate and is a hard yardstick.  At 1080 x 1920
 * LINEAR vec takes 1.3 - 1.9 x the copy and 0.27 - 0.56 x the general path; EDGE vec 1.8 - 3.6 x the copy and 0.18 - 0.30 x the general
 * path: EDGE is bound by the arithmetic of its five scores per pixel, not by memory.  At 480 x 720 a batch of 8 is 10 - 23 us of kernel, of
 * which the launch is a visible part.  vec is the faster path in every case measured, so it runs whenever its conditions hold.
 */
#ifndef CRTFX_DEINT_H
#define CRTFX_DEINT_H

#include <stddef.h>
#include <stdint.h>

#include "crtfx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crtfx_deint crtfx_deint;

/* the methods are stateless functions of one frame; the numbering leaves room for more */
typedef enum crtfx_deint_method { CRTFX_DEINT_LINEAR = 0, CRTFX_DEINT_EDGE = 1 } crtfx_deint_method;
typedef enum crtfx_deint_order { CRTFX_DEINT_TFF = 0, CRTFX_DEINT_BFF = 1 } crtfx_deint_order;
typedef enum crtfx_deint_fields { CRTFX_DEINT_FIRST = 0, CRTFX_DEINT_BOTH = 1 } crtfx_deint_fields;

/* Plans the deinterlacing of h x w x 3 frames of pix_fmt (CRTFX_PIX_U8 or CRTFX_PIX_F16) on `device` (the calling thread's current device
 * is restored).  CRTFX_E_INVALID: a null out pointer, h < 2 (a frame of two fields has two rows) or > 32767, w < 1 or > 32767, an unknown
 * pix_fmt, method, order or fields.  All of these are refused before a device is touched.  When it fails *out_plan is NULL and
 * crtfx_deint_last_error(NULL) holds the message (per calling thread), which names the offending field. */
int crtfx_deint_create(int device, int h, int w, int pix_fmt, int method, int order, int fields, crtfx_deint** out_plan);
int crtfx_deint_destroy(crtfx_deint* plan);
const char* crtfx_deint_last_error(const crtfx_deint* plan);

/* Output frames per source frame: 1 (FIRST) or 2 (BOTH); 0 for a null plan. */
int crtfx_deint_frames_out(const crtfx_deint* plan);

/* n SOURCE frames in one call: source frame i is read at src_base + i * src_stride_bytes, output frame j of the n * frames_out is written
 * at dst_base + j * dst_stride_bytes (h x w x 3 samples each, rows unpadded).  n = 0 does nothing.  CRTFX_E_INVALID: n < 0, a null frame
 * pointer, a stride shorter than a frame (the source's where n > 1, the destination's where more than one frame is written), an odd base
 * or stride for half frames, and a source range [src_base, src_base + (n - 1) * stride + frame) that overlaps the destination's.  Bytes
 * between frames are neither read nor written. */
int crtfx_deint_run(crtfx_deint* plan, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n,
                    void* stream);

/* Testing / A-B switches of one plan.  FORCE_GENERAL (0 / 1): take the general kernel whatever the width and alignment. */
typedef enum crtfx_deint_option { CRTFX_DEINT_OPT_FORCE_GENERAL = 1 } crtfx_deint_option;
int crtfx_deint_set_option(crtfx_deint* plan, int option, int value);

/* The path of the most recent crtfx_deint_run (before the first one: the path a run with aligned frames takes), frames = the SOURCE frames
 * of that run: `deint=k_deint<edge,u8,both,vec>;frames=5` or `deint=k_deint<linear,f16,first,general>;frames=5`. */
int crtfx_deint_last_plan(crtfx_deint* plan, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* CRTFX_DEINT_H */
