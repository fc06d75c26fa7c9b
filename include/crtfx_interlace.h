/*
 * crtfx_interlace.h — the interlace stage of libcrtfx.so, the delivery pair of the deinterlacers (crtfx_deint.h, crtfx_adeint.h): two
 * consecutive finished h x w x 3 RGB frames (CRTFX_PIX_U8 or CRTFX_PIX_F16) — the two fields of a chain that runs at field rate — are
 * woven into one interlaced frame on the device, with an optional vertical low-pass against line twitter.  It stands where a host pipeline
 * has `interlace` / `tinterlace` behind everything else: behind the delivery resize and the Canvas, which would mix the fields, at the
 * delivery size, in front of the Narrow and the egress plan (pythoncrt_amd/interlace.py, ends.py).
 *
 * Status codes (crtfx_status), pixel formats (crtfx_pixfmt) and conventions are those of crtfx.h: the caller owns every frame; work is
 * enqueued on the caller's hipStream_t (void*, NULL = the default stream); only destroy synchronises; the calling thread's current device
 * must be the plan's when it runs.  The stage depends on a device and five numbers, not on a crtfx_ctx: it has a handle of its own, the
 * handle owns no device memory, and it keeps nothing from one run to the next (every output frame is a function of two source frames of
 * the same run: pairs never reach across runs).
 *
 * Arithmetic, bit for bit; this is the library's own rule (tests/interlace_model.py restates it in numpy, tests/test_interlace_tables.py
 * and test_interlace_gpu.py hold the kernels to it with no differing element).  NOT claimed is equality with ffmpeg's `interlace`.
 * Output frame j is woven from the source frames A = 2 j and B = min(2 j + 1, n - 1): an odd last frame is woven with itself, so no
 * content is dropped.  The first field F1 is the even rows under CRTFX_INTERLACE_TFF and the odd rows under CRTFX_INTERLACE_BFF.  Output
 * row y comes from frame f = A if y % 2 is F1's parity, else from frame B, and r(k) is row clamp(y + k, 0, h - 1) of that SAME frame f:
 * the low-pass looks at the field's own progressive frame, never at the other one.  Integers are the codes 0..255 of uint8 frames; of half
 * frames the quarter codes q = rint_to_even(min(max(4 f, 0), 1020)), NaN -> 0 (the quantiser of crtfx_resize16.h), and a result r is
 * written as half(r / 4), which is exact (every quarter code is a half).  M is 255 for uint8 and 1020 for half.  Channels are independent.
 *     CRTFX_INTERLACE_NONE:     the row r(0) is copied as bits: every half pattern survives, NaN payloads included (as in crtfx_canvas.h)
 *     CRTFX_INTERLACE_LINEAR:   out = (r(-1) + 2 r(0) + r(1) + 2) >> 2
 *     CRTFX_INTERLACE_COMPLEX:  v = (-r(-2) + 2 r(-1) + 6 r(0) + 2 r(1) - r(2) + 4) >> 3      (an arithmetic shift: a floor)
 *                               v = min(max(v, 0), M)
 *                               out = max(v, r(0)) if r(-1) + r(1) > 2 r(0), else min(v, r(0))    (against over-sharpening)
 * Under LINEAR and COMPLEX every row is computed, so of half frames every row is quantised.  LINEAR needs no clamp (a weighted mean of
 * codes); COMPLEX's accumulator stays within -2040 .. 10204 on quarter codes (-510 .. 2554 on bytes), far inside an int.
 *
 * Frames: 3 bytes per pixel (uint8) or 6 (half), rows unpadded; the same sample type goes in and out.  n counts SOURCE frames and the
 * stage writes ceil(n / 2) frames; the destination stride is per OUTPUT frame.  For half frames every frame base and frame stride must
 * be even (CRTFX_E_INVALID otherwise); uint8 frames may start anywhere.
 *
 * This stage weaves RGB rows.  The chroma rows of a 4:2:0 delivery are formed behind it: by the box and the sited egress stages as a
 * progressive frame's are, so they mix the two fields, or — out_chroma_rows="interlaced" — by the field-paired egress stage
 * (crtfx_egress_field420.h) from rows of their own field only; 4:2:2, 4:4:4 and rgb24 deliveries have no such pairing.
 *
 * Paths; both give the same bytes, the path is chosen per run, and *_last_plan names the one that ran.  The order only selects a frame
 * pointer and is a launch argument: twelve builds.
 * k_interlace<lowpass,pix,vec>: runs where
 *     w % 8 == 0, both frame bases are multiples of 4, the source stride is a multiple of 4 (n > 1) and so is the destination's (more
 *     than one OUTPUT frame: n > 2)
 * — the rule of crtfx_deint.h.  One lane owns 1 row x 8 pixels of an OUTPUT frame, row y and columns 8 c .. 8 c + 7; all output frames of
 * a launch are one grid (grid.z; 32768 source frames per launch).  The lane reads that block of the 1, 3 or 5 rows r(k) of frame f as
 * dword-multiple loads at dword-aligned addresses (24 bytes: 16 + 8; 48 bytes of halves: 3 x 16) and stores its 24 results the same way.
 * k_interlace<lowpass,pix,general>: any size and alignment, and the CRTFX_INTERLACE_OPT_FORCE_GENERAL fallback: one lane per pixel of
 * an output frame; 1-byte (2-byte) loads and stores; grid = (pixels of a row, rows, output frames).
 * Every output element is written by exactly one lane on either path; row indices are clamped, not padded, so no byte outside a source
 * frame is read; bytes between frames are neither read nor written.
 *
 * Registers (gfx950, as built; tests/test_interlace_tables.py reads them from the library): VGPRs of k_interlace<lowpass,pix,path>
 *     k_interlace<none,u8,vec> 12, k_interlace<none,f16,vec> 18, k_interlace<linear,u8,vec> 28, k_interlace<linear,f16,vec> 44,
 *     k_interlace<complex,u8,vec> 43, k_interlace<complex,f16,vec> 57,
 *     k_interlace<none,u8,general> 5, k_interlace<none,f16,general> 5, k_interlace<linear,u8,general> 11, k_interlace<linear,f16,general> 12,
 *     k_interlace<complex,u8,general> 20, k_interlace<complex,f16,general> 22
 * (eight waves per SIMD for every build: the widest, <complex,f16,vec>, holds the 5 x 12 dwords of its five row blocks);
 * the general builds and the uint8 vec ones compute on integers, the half vec ones on the same integers held as floats;
 * no AGPRs, no LDS, no scratch, no spills.
 *
 * Kernel time per OUTPUT frame, measured once on one MI355X in batches of 8 output frames = 16 source frames (tools/interlace_kernel_times.py,
 * HIP events; profiles/interlace.txt holds the whole output), next to a device-to-device copy of equal traffic (the source bytes the stage
 * must read — one frame's under NONE, both frames whole under a low-pass — plus one frame written) and the untouched
 * k_deint<linear,pix,both,vec> per SOURCE frame of its own (one frame read, two written), all timed in the same run; us,
 * vec / general / copy / k_deint:
 *                            uint8                          half
 *     480 x 720    none      1.3 /  1.3 / 0.4 / 1.4         1.3 /  1.4 / 0.5 / 1.7
 *                  linear    1.4 /  2.1 / 0.5 / 1.4         1.5 /  2.2 / 1.0 / 1.7
 *                  complex   1.4 /  2.9 / 0.5 / 1.4         2.5 /  3.1 / 1.0 / 1.6
 *     1080 x 1920  none      2.0 /  6.1 / 1.6 / 4.4         4.1 /  6.4 / 3.5 / 8.9
 *                  linear    3.5 / 11.3 / 2.3 / 4.4         8.1 / 13.5 / 6.9 / 8.8
 *                  complex   5.1 / 16.9 / 2.3 / 4.4        14.6 / 18.8 / 6.9 / 8.9
 * Sixteen frames of either size lie in the Infinity Cache, so the copy runs above the HBM rate and is a hard yardstick.  At 1080 x 1920
 * NONE and LINEAR vec take 1.17 - 1.52 x the copy, and LINEAR 0.8 - 0.9 x k_deint's LINEAR, which moves the same three frames; COMPLEX vec
 * takes 2.2 x (uint8) and 2.1 x (half) the copy: it is bound by its arithmetic, five rows unpacked and, of halves, quantised per result.
 * (The half vec builds keep their codes as floats from the quantiser to half(r / 4) — every value is an integer below 2^24, so each step is
 * exact — and every filtered build forms its row addresses from one 64-bit product and 24-bit ones: with the integer form and a 64-bit
 * product per row <complex,f16,vec> took 18.0 us, as the general path does.)  The general path takes 1.3 - 3.3 x the vec path there.
 * At 480 x 720 a batch of 8 is 10 - 20 us of kernel, of which the launch is the visible part, and uint8 NONE is a tie: 1.311 us on the vec
 * path against 1.306 on the general one (from the rates the profile prints), 0.4 % apart and inside the spread between two runs, which
 * saw it either way round.  Everywhere else vec is the faster path, at 1080 x 1920 by 1.3 x at the least, and nowhere is the general path
 * measurably faster: vec runs whenever its conditions hold.
 */
#ifndef CRTFX_INTERLACE_H
#define CRTFX_INTERLACE_H

#include <stddef.h>
#include <stdint.h>

#include "crtfx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crtfx_interlace crtfx_interlace;

typedef enum crtfx_interlace_order { CRTFX_INTERLACE_TFF = 0, CRTFX_INTERLACE_BFF = 1 } crtfx_interlace_order;
typedef enum crtfx_interlace_lowpass { CRTFX_INTERLACE_NONE = 0, CRTFX_INTERLACE_LINEAR = 1, CRTFX_INTERLACE_COMPLEX = 2 } crtfx_interlace_lowpass;

/* Plans the interlacing of h x w x 3 frames of pix_fmt (CRTFX_PIX_U8 or CRTFX_PIX_F16) on `device` (the calling thread's current device
 * is restored).  CRTFX_E_INVALID: a null out pointer, h < 2 (a frame of two fields has two rows) or > 32767, w < 1 or > 32767, an unknown
 * pix_fmt, order or lowpass.  All of these are refused before a device is touched.  When it fails *out_plan is NULL and
 * crtfx_interlace_last_error(NULL) holds the message (per calling thread), which names the offending field. */
int crtfx_interlace_create(int device, int h, int w, int pix_fmt, int order, int lowpass, crtfx_interlace** out_plan);
int crtfx_interlace_destroy(crtfx_interlace* plan);
const char* crtfx_interlace_last_error(const crtfx_interlace* plan);

/* Source frames per output frame: 2; 0 for a null plan. */
int crtfx_interlace_frames_in(const crtfx_interlace* plan);

/* n SOURCE frames in one call: source frame i is read at src_base + i * src_stride_bytes, output frame j of the ceil(n / 2) is written at
 * dst_base + j * dst_stride_bytes (h x w x 3 samples each, rows unpadded).  n = 0 does nothing.  CRTFX_E_INVALID: n < 0, a null frame
 * pointer, a stride shorter than a frame (the source's where n > 1, the destination's where more than one frame is written), an odd base
 * or stride for half frames, and a source range [src_base, src_base + (n - 1) * stride + frame) that overlaps the destination's range of
 * ceil(n / 2) frames.  Bytes between frames are neither read nor written. */
int crtfx_interlace_run(crtfx_interlace* plan, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n,
                        void* stream);

/* Testing / A-B switches of one plan.  FORCE_GENERAL (0 / 1): take the general kernel whatever the width and alignment. */
typedef enum crtfx_interlace_option { CRTFX_INTERLACE_OPT_FORCE_GENERAL = 1 } crtfx_interlace_option;
int crtfx_interlace_set_option(crtfx_interlace* plan, int option, int value);

/* The path of the most recent crtfx_interlace_run (before the first one: the path a run with aligned frames takes), frames = the SOURCE
 * frames of that run: `interlace=k_interlace<linear,u8,vec>;frames=6` or `interlace=k_interlace<none,f16,general>;frames=5`. */
int crtfx_interlace_last_plan(crtfx_interlace* plan, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* CRTFX_INTERLACE_H */
