/*
 * crtfx_lut3d.h — the 3D LUT stage of libcrtfx.so: h x w x 3 RGB frames, uint8 (CRTFX_PIX_U8) or half (CRTFX_PIX_F16, IEEE half on the
 * 0..255 scale), go through a colour cube of edge N with tetrahedral interpolation on the device.  It stands where a host pipeline has
 * `lut3d=`: directly in front of the chain (a log or PQ source brought to display-referred video) and directly behind it (a display or
 * creative transform), at render size and on the chain's pixel type (pythoncrt_amd/lut3d.py, ends.py).  The cube is what a `.cube` file
 * holds (pythoncrt_amd/cube.py reads one); the stage has no transfer-function or primaries code of its own.
 *
 * Status codes (crtfx_status), pixel formats (crtfx_pixfmt) and conventions are those of crtfx.h: the caller owns every frame; work is
 * enqueued on the caller's hipStream_t (void*, NULL = the default stream); only create / destroy / set_table synchronise; the calling
 * thread's current device must be the plan's when it runs.  The stage depends on a device, a size, a pixel type and a cube, not on a
 * crtfx_ctx: it has a handle of its own, and the handle owns the packed cube in device memory.
 *
 * Arithmetic, bit for bit (tests/lut3d_model.py restates it in numpy, tests/test_lut3d_tables.py and test_lut3d_gpu.py hold the kernels
 * to it with no differing element).
 * The cube: entry T[b][g][r][c], red fastest as in the file, is a quarter code 0..CRTFX_LUT3D_QMAX (1020) — the scale of crtfx_deep.h and
 * crtfx_resize16.h, q / 4 on the 0..255 scale, every one a half — made on the host as rint_to_even(1020 * min(max(v, 0), 1)) in float64
 * from the file's value v.  `table` is uint16[N^3 * 3] in that order; 2 <= N <= CRTFX_LUT3D_MAX_N (65).
 * Input per channel, on scale S:
 *     uint8 frames:  x = u, S = 255
 *     half frames:   x = q = rint_to_even(min(max(4 * float(half), 0), 1020)), NaN -> 0, S = 1020      (crtfx_resize16.h's `in:` quantiser:
 *                    -0, negatives, -inf -> 0; +inf -> 1020)
 * Per pixel and per channel c:
 *     num_c = x_c * (N - 1)
 *     i_c   = min(num_c / S, N - 2)          integer division
 *     f_c   = num_c - i_c * S                0..S; S only at x_c = S
 * Tetrahedral interpolation: the three channels ordered by f descending, f1 >= f2 >= f3 with their unit steps e1, e2, e3 in the cube;
 * for each output channel
 *     sum = (S - f1) * T[i] + (f1 - f2) * T[i + e1] + (f2 - f3) * T[i + e1 + e2] + f3 * T[i + (1, 1, 1)]
 *     out = (sum + 510) / 1020               integer division
 * With uint8 the weights sum to 255 and out is a uint8 code; with halves they sum to 1020, out is a quarter code and half(out / 4) is
 * written, exactly.  sum <= 1020 * 1020, so 32-bit arithmetic never wraps (and every product fits 24 bits).  Ties between fractions need
 * no rule: the weight between two equal fractions is 0, so every order of equal fractions gives the same sum.  A quantised identity cube
 * returns every uint8 code and every quarter code unchanged for every N the tests try (2..5, 9, 16..18, 32..35, 64, 65).
 * Only tetrahedral interpolation exists; entries and results are quarter codes, so a cube's precision here is 10 bits.
 *
 * Frames: rows unpadded, 3 bytes per pixel (uint8) or 6 (half); the operation is pointwise, so a frame is a flat list of h * w pixels and
 * nothing is asked of w.  Half frame bases and strides must be even (CRTFX_E_INVALID otherwise); uint8 frames may start anywhere.
 *
 * Where the cube lives.  The plan packs an entry into one dword, r | g << 10 | b << 20, and owns that table in device memory.
 * lds:    N <= CRTFX_LUT3D_LDS_MAX_N (34): N^3 dwords are at most 157 216 of the CU's CRTFX_LUT3D_LDS_BYTES (163 840; 35^3 dwords are
 *         171 500 and do not fit); N = 33, the common size, takes 143 748.  Every block copies the packed table into dynamic LDS once
 *         (above 64 KiB the kernel function's dynamic-LDS limit is raised at create, always to the CU's 163 840 and never lowered: the
 *         limit is the function's, not the plan's, and plans of different N live side by side) and then grid-strides over the pixels of ALL n frames of the
 *         run, so the copy is paid once per block per launch.  Footprint rule: blocks of 1024 lanes, grid = CUs x min(163 840 / (4 N^3), 2)
 *         — two blocks fill a CU's 2048 lanes; a cube of more than 81 920 bytes (N >= 28) leaves room for one — and never more blocks than
 *         the run has work for.  A pixel costs four ds_read_b32 gathers and integer VALU work.
 * global: the same gathers from the device table, which stays L2-resident (65^3 dwords are 1.1 MB).  It serves N = 35..65, and
 *         CRTFX_LUT3D_OPT_FORCE_GLOBAL selects it for A/B.  Grid = CUs x 2 blocks of 1024 lanes, at most the run's work.
 * How a lane walks pixels.
 * vec:     a lane owns 4 consecutive pixels: for uint8 three dword loads and three dword stores, for halves one 16-byte and one 8-byte
 *          load and store, all at dword-aligned addresses.  It runs where both frame bases are multiples of 4 and (n > 1) both frame strides
 *          are multiples of 4.  The last 1..3 pixels of a frame go element by element, in the lane that would own their chunk.
 * general: one lane per pixel with 1-byte (2-byte) loads and stores: any alignment, and the CRTFX_LUT3D_OPT_FORCE_GENERAL fallback.
 * All paths give the same bits; the path is chosen per run and *_last_plan names the one that ran.  No element outside a frame is read or
 * written; every destination element is written by exactly one lane; bytes between frames are neither read nor written.
 *
 * Builds: k_lut3d<sample, table, walk> — four (lds | global) x (vec | general) by two sample types (u8 | half).
 * Registers (gfx950, as built; tests/test_lut3d_tables.py reads them from the library and holds every build to 64 VGPRs + AGPRs, two
 * blocks of 1024 lanes per CU):
 * k_lut3d<u8,lds,vec> 30 VGPRs, k_lut3d<u8,lds,general> 28, k_lut3d<u8,global,vec> 42, k_lut3d<u8,global,general> 29,
 * k_lut3d<half,lds,vec> 55, k_lut3d<half,lds,general> 28, k_lut3d<half,global,vec> 55, k_lut3d<half,global,general> 29;
 * no AGPRs, no static LDS (the lds builds' block is dynamic: its size is the plan's `lds`), no scratch, no spills.
 *
 * Kernel time per frame, measured once on one MI355X in batches of 8 (tools/lut3d_kernel_times.py, HIP events; profiles/lut3d.txt holds the
 * whole output), random cubes and random frames — the worst case for the gathers — next to a device-to-device copy of the same traffic (a
 * frame read + a frame written) timed in the same run; us per frame, vec / general:
 *                      uint8  lds           global          copy      half   lds           global          copy
 *     1080p  N = 17           5.1 /  5.9     9.5 /  12.8     1.6              6.7 /  7.0    10.2 /  12.9     3.0
 *            N = 33           5.7 /  6.8    21.8 /  23.1     1.6              7.3 /  8.0    21.5 /  23.4     3.0
 *            N = 65                         27.3 /  27.4     1.6                            26.2 /  27.6     3.0
 *     4K     N = 17          20.1 / 23.8    37.9 /  52.2     9.3             27.2 / 30.5    50.7 /  56.9    19.9
 *            N = 33          22.3 / 29.0    92.3 / 115.0     9.3             30.1 / 35.6    94.6 / 120.1    19.7
 *            N = 65                        112.8 / 129.1     9.3                           111.2 / 133.0    19.9
 * lds is the faster table path in every case measured — 1.5 - 1.9 x faster than global at N = 17, 2.9 - 4.1 x at N = 33, at both sizes and
 * on both sample types — so it is the default for every N it holds (N <= 34), and global serves N = 35..65 only.  lds + vec takes 1.4 - 3.6 x
 * the copy (4K half 1.37 - 1.53 x; 1080p uint8 3.2 - 3.6 x, against a hard yardstick: a 1080p batch, 8 frames in and 8 out, is
 * cache-resident — it lies in the Infinity Cache and its copy runs at 7.8 - 8.4 TB/s, not at HBM's rate; four gathers and some sixty integer instructions per pixel against 6 or 12 bytes
 * moved); general takes 1.04 - 1.30 x the vec walk on the lds path.  On the global path the gathers' L2 traffic sets the time: it grows with
 * the cube (N = 17 -> 33: 1.9 - 2.4 x) and hardly with the sample type.
 */
#ifndef CRTFX_LUT3D_H
#define CRTFX_LUT3D_H

#include <stddef.h>
#include <stdint.h>

#include "crtfx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crtfx_lut3d crtfx_lut3d;

#define CRTFX_LUT3D_QMAX 1020           /* the largest entry: quarter code of 255 */
#define CRTFX_LUT3D_MIN_N 2
#define CRTFX_LUT3D_MAX_N 65
#define CRTFX_LUT3D_LDS_MAX_N 34        /* the largest cube the lds path holds: 4 * 34^3 = 157 216 <= 163 840 < 4 * 35^3 = 171 500 */
#define CRTFX_LUT3D_LDS_BYTES 163840    /* LDS of one CU */

/* Plans the cube for h x w x 3 frames of pix_fmt (CRTFX_PIX_U8 or CRTFX_PIX_F16) on `device`, packs `table` (uint16[N^3 * 3], above) and
 * copies it to the device (synchronises; the calling thread's current device is restored).  CRTFX_E_INVALID: a null out pointer, an unknown
 * pix_fmt, h or w < 1 or > 32767, N outside 2..65, a null table, an entry above 1020.  All of these are refused before a device is touched.
 * When it fails *out_plan is NULL and crtfx_lut3d_last_error(NULL) holds the message (per calling thread), which names the offending field. */
int crtfx_lut3d_create(int device, int h, int w, int pix_fmt, int N, const uint16_t* table, crtfx_lut3d** out_plan);
int crtfx_lut3d_destroy(crtfx_lut3d* plan);
const char* crtfx_lut3d_last_error(const crtfx_lut3d* plan);

/* n frames in one call: frame i is read at src_base + i * src_stride_bytes and written at dst_base + i * dst_stride_bytes (h x w x 3
 * samples of the plan's type each, rows unpadded).  n = 0 does nothing.  CRTFX_E_INVALID: n < 0, a null frame pointer, a stride shorter
 * than a frame (n > 1), an odd base or stride of half frames, and a source range [src_base, src_base + (n - 1) * stride + frame) that
 * overlaps the destination's.  Bytes between frames are neither read nor written. */
int crtfx_lut3d_run(crtfx_lut3d* plan, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n,
                    void* stream);

/* Swaps the cube of a live plan (synchronises: the runs already enqueued finish with the old cube).  CRTFX_E_INVALID: an N other than
 * the plan's, a null table, an entry above 1020 — the plan keeps its cube. */
int crtfx_lut3d_set_table(crtfx_lut3d* plan, int N, const uint16_t* table);

/* Testing / A-B switches of one plan.  FORCE_GENERAL (0 / 1): one lane per pixel whatever the alignment.  FORCE_GLOBAL (0 / 1): gather from
 * the device table whatever N. */
typedef enum crtfx_lut3d_option { CRTFX_LUT3D_OPT_FORCE_GENERAL = 1, CRTFX_LUT3D_OPT_FORCE_GLOBAL = 2 } crtfx_lut3d_option;
int crtfx_lut3d_set_option(crtfx_lut3d* plan, int option, int value);

/* The path of the most recent crtfx_lut3d_run (before the first one: the path a run with aligned frames takes):
 * `lut3d=k_lut3d<u8,lds,vec>;n=33;lds=143748;frames=5`, `lut3d=k_lut3d<half,global,general>;n=65;lds=0;frames=5`. */
int crtfx_lut3d_last_plan(crtfx_lut3d* plan, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* CRTFX_LUT3D_H */
