/*
 * crtfx_canvas.h — the geometry stage of libcrtfx.so: one window of an h x w x 3 RGB frame (CRTFX_PIX_U8 or CRTFX_PIX_F16) is moved to one
 * place of a frame of another size on the device, and the rest of that frame is filled with a colour.  It stands where a host pipeline has
 * `crop` and `pad`: in front of the chain it cuts the picture area out of a letterboxed source, behind it it centres a 4:3 render on a 16:9
 * canvas or cuts the centre of a wide render (pythoncrt_amd/canvas.py, ends.py).
 *
 * Status codes (crtfx_status), pixel formats (crtfx_pixfmt) and conventions are those of crtfx.h: the caller owns every frame; work is
 * enqueued on the caller's hipStream_t (void*, NULL = the default stream); only destroy synchronises; the calling thread's current device
 * must be the plan's when it runs.  The stage depends on a device and twelve numbers, not on a crtfx_ctx: it has a handle of its own, and
 * the handle owns no device memory.
 *
 * Arithmetic: none.  With frames of src_h x src_w x 3 and dst_h x dst_w x 3 samples, rows unpadded,
 *     dst[i][y][x][c] = src[i][win_y + y - dst_y][win_x + x - dst_x][c]    if dst_y <= y < dst_y + win_h and dst_x <= x < dst_x + win_w
 *                     = fill[c]                                             otherwise
 * Samples are copied as bits: every half pattern survives, NaN payloads included.  fill[c] is a code 0..255 for uint8 frames and the
 * half's bit pattern for half frames.  A pure crop has dst = window and dst_y = dst_x = 0; a pure pad has window = the whole source; one
 * plan can do both.
 *
 * Frames: 3 bytes per pixel (uint8) or 6 (half).  For half frames every frame base and frame stride must be even (CRTFX_E_INVALID
 * otherwise); uint8 frames may start anywhere.
 *
 * Paths; both give the same bytes, the path is chosen per run, and *_last_plan names the one that ran.
 * k_canvas<.,vec>: the destination frame is cut into aligned 16-byte chunks of its own bytes, one lane per chunk, all n frames in one grid
 * (grid.z).  It runs where
 *     the destination base is a multiple of 4, the destination stride is a multiple of 4 (n > 1),
 *     the destination frame's bytes are a multiple of 4, and both frames are shorter than 2^31 bytes
 * — nothing is asked of the source: a window starts at an arbitrary byte of an arbitrarily placed frame.  Every store is an aligned
 * dword-multiple store: one 16-byte store per lane where the destination base and stride are multiples of 16, four dword stores otherwise,
 * and dword stores for the last chunk of a frame whose bytes are no multiple of 16.  A chunk that lies inside the window is read as the
 * four or five ALIGNED dwords (one 16-byte load at a dword-aligned address plus, where the source address is off a dword, one dword) that
 * cover its 16 source bytes, brought into place by a funnel shift (v_alignbit_b32).  A chunk that lies in a bar is three dwords of the
 * 12-byte periodic pattern of the fill colour, rotated by the chunk's index modulo 3.  A chunk that straddles a window edge is taken dword
 * by dword the same way (two aligned dwords and a funnel shift, or one pattern dword) from the chunk's own row and column, and a dword
 * that straddles the edge is assembled from byte loads and pattern bytes; a chunk that straddles a row end or is the frame's last, short
 * one does the same with a division per dword, and per byte for the dword the row ends in.
 * No byte outside a source frame is read.  Aligned loads round the source address down and the end up, so the first and the last dword of
 * a frame may stick out of it when the frame's base or size is off a dword: before every aligned load the kernel compares the load's
 * extent, as offsets into the frame, [s - (address & 3), + 16 | 20 | 8) with [0, frame bytes), and a chunk or dword whose aligned extent is
 * not inside takes the next narrower form — in the end byte loads at the exact offsets s .. s + 3, which are inside because the window is.
 * k_canvas<.,general>: any size and alignment, and the CRTFX_CANVAS_OPT_FORCE_GENERAL fallback: one lane per destination sample, one
 * 1-byte (uint8) or 2-byte (half) load or none, one store of that width; grid = (row samples, rows, frames).
 * Every destination element is written by exactly one lane on either path; bytes between frames are neither read nor written.
 *
 * Registers (gfx950, as built; tests/test_canvas_tables.py reads them from the library and holds every build to 64 VGPRs + AGPRs):
 * k_canvas<u8,vec> 24 VGPRs, k_canvas<f16,vec> 24, k_canvas<u8,general> 4, k_canvas<f16,general> 4 (eight waves per SIMD each); no AGPRs, no LDS, no scratch, no
 * spills.
 *
 * Kernel time per frame, measured once on one MI355X in batches of 8 (tools/canvas_kernel_times.py, HIP events; profiles/canvas.txt holds the
 * whole output), uint8 / half, next to a device-to-device copy of the same traffic (window bytes read + canvas bytes written) timed in the
 * same run:
 *     pad 2160 x 2880 -> 2160 x 3840            vec  7.2 / 14.2 us   general 42.6 / 50.6   copy  8.1 / 16.0   vec = 0.89 / 0.89 x the copy
 *     pad 1080 x 1440 -> 1080 x 1920, dx = 240  vec  1.8 /  3.3      general  8.8 /  9.3   copy  1.6 /  2.6   vec = 1.10 / 1.25 x
 *     the same at dx = 241 (misaligned)         vec  2.1 /  3.4      general  8.8 /  9.2   copy  1.6 /  2.6   vec = 1.30 / 1.28 x
 *     crop 1600 x 3840 at y = 280 of 2160 x 3840   vec  5.8 / 12.5   general 32.8 / 40.9   copy  6.6 / 13.6   vec = 0.89 / 0.92 x
 *     crop 2160 x 2880 at x = 481 of 2160 x 3840   vec  6.1 / 12.9   general 32.7 / 41.8   copy  6.8 / 13.8   vec = 0.91 / 0.94 x
 * The general path takes 3.0 - 5.4 x the copy and 2.7 - 5.9 x the vec path; vec is the faster one in every case measured, so it runs whenever
 * its conditions hold.  A misaligned SOURCE costs nothing that shows (the crop at x = 481); a misaligned PLACEMENT costs a fifth at uint8
 * (dx = 241 against 240: two chunks of every row straddle a window edge and take the dword-by-dword form while the rest of their wave
 * waits; with a division per dword in that form, as first built, the same case took 3.0 / 4.1 us).
 */
#ifndef CRTFX_CANVAS_H
#define CRTFX_CANVAS_H

#include <stddef.h>
#include <stdint.h>

#include "crtfx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crtfx_canvas crtfx_canvas;

/* Plans the move on `device` (the calling thread's current device is restored).  pix_fmt: CRTFX_PIX_U8 or CRTFX_PIX_F16.
 * CRTFX_E_INVALID: an unknown pixel format, a null `fill` or out pointer, a size (src_h, src_w, win_h, win_w, dst_h, dst_w) < 1 or
 * > 32767, a window that leaves the source (win_y, win_x < 0, win_y + win_h > src_h, win_x + win_w > src_w), a placement that leaves the
 * destination (dst_y, dst_x < 0, dst_y + win_h > dst_h, dst_x + win_w > dst_w), a uint8 fill > 255.  All of these are refused before a
 * device is touched.  When it fails *out_plan is NULL and crtfx_canvas_last_error(NULL) holds the message (per calling thread), which
 * names the offending field. */
int crtfx_canvas_create(int device, int pix_fmt, int src_h, int src_w, int win_y, int win_x, int win_h, int win_w,
                        int dst_h, int dst_w, int dst_y, int dst_x, const uint16_t fill[3], crtfx_canvas** out_plan);
int crtfx_canvas_destroy(crtfx_canvas* plan);
const char* crtfx_canvas_last_error(const crtfx_canvas* plan);

/* n frames in one call: frame i is read at src_base + i * src_stride_bytes (src_h x src_w x 3 samples, rows unpadded) and written at
 * dst_base + i * dst_stride_bytes (dst_h x dst_w x 3 samples).  n = 0 does nothing.  CRTFX_E_INVALID: n < 0, a null frame pointer, a
 * stride shorter than a frame (n > 1), an odd base or stride for half frames, and a source range [src_base, src_base + (n - 1) * stride +
 * frame) that overlaps the destination's.  Bytes between frames are neither read nor written. */
int crtfx_canvas_run(crtfx_canvas* plan, const void* src_base, size_t src_stride_bytes, void* dst_base,
                     size_t dst_stride_bytes, int n, void* stream);

/* Testing / A-B switches of one plan.  FORCE_GENERAL (0 / 1): take k_canvas<.,general> whatever the alignment. */
typedef enum crtfx_canvas_option { CRTFX_CANVAS_OPT_FORCE_GENERAL = 1 } crtfx_canvas_option;
int crtfx_canvas_set_option(crtfx_canvas* plan, int option, int value);

/* The path of the most recent crtfx_canvas_run (before the first one: the path a run with aligned frames takes):
 * `canvas=k_canvas<u8,vec>;frames=5` or `canvas=k_canvas<f16,general>;frames=5`. */
int crtfx_canvas_last_plan(crtfx_canvas* plan, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* CRTFX_CANVAS_H */
