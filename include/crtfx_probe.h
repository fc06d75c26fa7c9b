/*
 * crtfx_probe.h — the source probe of libcrtfx.so: it MEASURES what the keywords in front of the chain describe.  An h x w x 3 RGB frame
 * (CRTFX_PIX_U8 or CRTFX_PIX_F16), as a source plan writes it, gives one small record of exact integer statistics, on the device: channel
 * extremes, luma sum, luma histogram, row and column sums of luma, and three comb sums that tell a woven frame's field order.  The host layer
 * (pythoncrt_amd/probe.py) turns the records of a stream into `in_crop`, `deinterlace` / `field_order` and the levels — what a separate
 * cropdetect / idet / signalstats pass in front of the pipeline did.  It changes no frame and stands in no chain.
 *
 * Status codes, pixel formats and conventions are those of crtfx.h and crtfx_adeint.h: the caller owns every frame, the previous one
 * included, and the records; work is enqueued on the caller's hipStream_t; only destroy synchronises; the calling thread's current device must
 * be the plan's when it runs.  The handle owns no device memory and keeps nothing from one run to the next: the previous frame of a run's first
 * frame is an argument of that run.
 *
 * Arithmetic, word for word; this is the library's own rule (tests/probe_model.py restates it in numpy, tests/test_probe_tables.py and
 * test_probe_gpu.py hold the kernels to it with no differing word).  NOT claimed is equality with any other filter, ffmpeg's cropdetect,
 * idet and signalstats included.
 * Codes.  A uint8 sample u has the code q = 4 u.  A half sample has the family's quarter-code quantiser, the one crtfx_lut3d.h and
 * crtfx_resize16.h state: q = rint_to_even(min(max(4 f, 0), 1020)), NaN -> 0.  Every code lies in 0..1020.
 * Luma of a pixel: Y = (54 r + 183 g + 19 b + 128) >> 8 on codes.  The weights sum to 256, so Y lies in 0..1020.
 * The record of frame i is crtfx_probe_words(h, w) = 272 + h + w, rounded up to even, uint32 words; a 64-bit sum sits at an even word offset,
 * low word first:
 *     word 0          flags: bit 0 = the frame had a previous frame
 *     words 1..6      min r, min g, min b, max r, max g, max b (codes)
 *     word 7          0
 *     words 8..9      the sum of Y over the frame
 *     words 10..11    S_cur  = the sum over rows y = 1..h-2 and every x of |Y[y-1][x] + Y[y+1][x] - 2 Y[y][x]|, all three rows the frame's own
 *     words 12..13    S_even = the same sum over the EVEN rows y of that range only, with row y taken from the PREVIOUS frame; 0 without one
 *     words 14..15    S_odd  = likewise over the odd rows
 *     words 16..271   histogram of Y >> 2, 256 bins (the counts sum to h w)
 *     words 272..272+h-1        row sums of Y
 *     words 272+h..272+h+w-1    column sums of Y
 * and a last word of 0 where 272 + h + w is odd.  With h < 3 the three S sums are 0.
 * The previous frame of frame i > 0 is frame i - 1 of the batch; that of frame 0 is prev_frame, or none where it is NULL.
 * Bounds: a row or column sum is <= 32767 * 1020 < 2^32; a histogram bin is <= 32767^2 < 2^32; the sum of Y is <= 32767^2 * 1020 < 2^41 and
 * an S sum <= 32767^2 * 2040 < 2^42: those four take 64 bits.  Every sum is an integer sum, so the result does not depend on the order in
 * which the kernels' atomic adds arrive: a run gives the same words every time.
 * Why S_even and S_odd tell the field order: under TFF an even row of the previous frame is three field times from the current odd rows
 * around it and an odd row is one field time from its even neighbours, so where the picture moves S_even exceeds S_odd; BFF mirrors this; a
 * progressive or still source shows no parity asymmetry.  On the 24 x 40 field-rate scenes of tests/probe_model.py (vertical grey stripes that
 * move one pixel per field), summed over five frame pairs: woven TFF S_cur / S_even / S_odd = 973 280 / 1 162 040 / 486 640, woven BFF
 * 973 280 / 486 640 / 1 162 040, progressive 0 / 846 120 / 846 120, still 0 / 0 / 0.  With an odd h there is one more odd interior row than
 * even ones, which alone tilts the two sums by (h - 1) / (h - 3).
 *
 * Frames: 3 or 6 bytes per pixel, rows unpadded, n frames src_stride_bytes apart, half frames need even bases and strides; prev_frame is one
 * frame of h x w x 3 samples.  Records: n records record_stride_bytes apart; the base and (n > 1) the stride are multiples of 8.
 * crtfx_probe_run initialises the records itself, on the caller's stream: running twice into one buffer gives the same words.  It writes no
 * byte outside [record, record + 4 words) of each frame.
 *
 * Paths; both give the same words, the path is chosen per run, and *_last_plan names the one that ran.
 * k_probe_init: one lane per word of every record of the launch: the flags, the minima at 0xffffffff, zeros.
 * k_probe<pix,vec>: runs where w % 8 == 0, the source base is a multiple of 4, the source stride is (n > 1), and prev_frame, when it is not
 *     NULL, is.  One lane owns 8 pixels of a row; every load is a dword-multiple access at a dword-aligned address, as k_adeint<...,vec>'s.  A
 *     block of 256 lanes owns a tile of 32 rows x 512 columns: each of its four waves walks 8 consecutive rows top to bottom with the luma of
 *     rows y - 1, y, y + 1 in registers — a one-row halo above and below — so one pass reads each source frame once (plus the halo rows) and
 *     row y of the previous frame, which is the batch's own frame i - 1 and comes from the caches.  All n frames are one grid (grid.z).
 * k_probe<pix,general>: any size and alignment, and the CRTFX_PROBE_OPT_FORCE_GENERAL fallback: the same block with one lane per pixel (a
 *     tile of 32 rows x 64 columns), 1-byte (2-byte) loads.
 * Global atomics of a block are bounded by its tile, not by its content: the histogram is accumulated in LDS — sixteen lane-interleaved
 * sub-histograms (16 KiB), and a wave whose 64 lanes hold ONE bin (a flat picture) adds their count once instead of 64 times — and flushed
 * once per block, at most one add per bin; a row sum is reduced across the wave and added once per row per wave; column sums are kept in
 * registers down the wave's rows, joined across the four waves in LDS and added once per column per block; the extremes, the sum of Y and
 * the S sums are reduced across the block and cost one atomic each (atomicAdd(unsigned long long*) for the 64-bit ones).  A lane's partial
 * sums stay below 2^18, a block's below 2^26.  A launch covers at most 32 768 frames; the first frame of a later launch takes the last
 * frame of the launch before it as its previous frame.
 *
 * Registers and LDS (gfx950, as built; tests/test_probe_tables.py reads them from the library): VGPRs / LDS bytes of k_probe<pix,path>
 *     k_probe<u8,vec> 90 / 18592, k_probe<f16,vec> 90 / 18592, k_probe<u8,general> 42 / 16800, k_probe<f16,general> 44 / 16800
 * (five waves per SIMD for the vec builds, eight for the general ones; the LDS is the 16 KiB of sub-histograms, a tile's column sums and 160 bytes);
 * no AGPRs, no scratch, no spills; k_probe_init uses no LDS.
 *
 * Kernel time per frame, k_probe_init included, measured once on one MI355X in batches of 8 in which every frame has a previous frame
 * (tools/probe_kernel_times.py, HIP events; profiles/probe.txt holds the whole output), next to two yardsticks timed in the same run: the
 * untouched k_adeint<pix,first,vec>, which reads the same frames and writes them too, and a device-to-device copy of the frames; three
 * contents — random noise, ONE value (every lane of every wave the same bin: the atomics' worst case), black bars around noise with a moving
 * block; us, vec / general / adeint vec / copy:
 *                            uint8                          half
 *     480 x 720    random    2.7 /  3.4 / 2.4 / 0.4         3.1 /  3.7 /  3.7 / 0.5
 *                  constant  2.6 /  3.1 / 2.3 / 0.4         3.1 /  3.4 /  3.7 / 0.5
 *                  boxed     2.7 /  3.2 / 2.4 / 0.4         3.1 /  3.5 /  3.7 / 0.5
 *     1080 x 1920  random    5.3 / 18.0 / 8.0 / 1.8         7.2 / 19.0 / 13.4 / 3.5
 *                  constant  5.2 / 18.7 / 7.9 / 1.8         7.1 / 19.7 / 13.4 / 3.5
 *                  boxed     5.1 / 15.7 / 7.9 / 1.8         7.1 / 16.8 / 13.3 / 3.4
 * Eight frames of either size lie in the Infinity Cache, so the copy is a hard yardstick.  The constant frame costs what the random one
 * costs, within 0.1 us: the content does not show in the time.  The vec path takes 0.53 - 0.66 x k_adeint's vec path at 1080 x 1920 and
 * 0.83 - 1.14 x at 480 x 720, where a batch is 240 blocks on 256 compute units and two launches; it takes 2.0 - 2.9 x the copy at the large
 * size and 5.8 - 6.8 x at the small one.  vec takes 0.28 - 0.42 x the general path at 1080 x 1920 and 0.80 - 0.91 x at 480 x 720: it is the
 * faster path in every case measured, so it runs whenever its conditions hold.
 */
#ifndef CRTFX_PROBE_H
#define CRTFX_PROBE_H

#include <stddef.h>
#include <stdint.h>

#include "crtfx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crtfx_probe crtfx_probe;

/* Plans the probe of h x w x 3 frames of pix_fmt (CRTFX_PIX_U8 or CRTFX_PIX_F16) on `device` (the calling thread's current device is
 * restored).  CRTFX_E_INVALID: a null out pointer, h or w outside 1..32767 (h = 1 is allowed), an unknown pix_fmt — before a device is
 * touched.  When it fails *out_plan is NULL and crtfx_probe_last_error(NULL) holds the message (per calling thread), which names the field. */
int crtfx_probe_create(int device, int h, int w, int pix_fmt, crtfx_probe** out_plan);
int crtfx_probe_destroy(crtfx_probe* plan);
const char* crtfx_probe_last_error(const crtfx_probe* plan);

/* uint32 words of one record: 272 + h + w rounded up to even; 0 for h or w outside 1..32767.  Needs no plan. */
size_t crtfx_probe_words(int h, int w);

/* n frames in one call, one record each.  prev_frame is the frame in front of frame 0, or NULL: frame 0 then has no previous frame, its
 * flags are 0 and its S_even and S_odd are 0.  n = 0 does nothing.  CRTFX_E_INVALID: a negative n, a null pointer, odd bases or strides of
 * half frames or an odd prev_frame, a record base or (n > 1) record stride that is not a multiple of 8, strides smaller than a frame or a
 * record, records that overlap the source range or [prev_frame, prev_frame + frame), the wrong current device.  prev_frame may lie anywhere
 * else, inside the source range included. */
int crtfx_probe_run(crtfx_probe* plan, const void* prev_frame, const void* src_base, size_t src_stride_bytes, void* records,
                    size_t record_stride_bytes, int n, void* stream);

/* Testing / A-B switches of one plan.  FORCE_GENERAL (0 / 1): take the general kernel whatever the width and alignment. */
typedef enum crtfx_probe_option { CRTFX_PROBE_OPT_FORCE_GENERAL = 1 } crtfx_probe_option;
int crtfx_probe_set_option(crtfx_probe* plan, int option, int value);

/* The path of the most recent crtfx_probe_run (before the first one: the path a run with aligned frames takes), frames = the frames of that
 * run: `probe=k_probe<u8,vec>;frames=5`. */
int crtfx_probe_last_plan(crtfx_probe* plan, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* CRTFX_PROBE_H */
