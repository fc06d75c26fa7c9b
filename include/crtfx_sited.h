/*
 * crtfx_sited.h — the sited source stage of libcrtfx.so: the seven sub-sampled source formats the other source stages read (crtfx_unpack_*,
 * crtfx_unpack422_*, crtfx_unpack10_*) converted to RGB with the chroma planes INTERPOLATED at a stated siting instead of replicated over
 * their pixels.  Replication puts 2-pixel-wide colour steps on every saturated edge and, for the chroma siting of MPEG-2 / H.264 / HEVC
 * streams ("left", what ffprobe reports for almost every file), shifts colour by a quarter luma pixel against luma.  The stage stands where
 * the replicating one stood: same frames in, same RGB frames out, the same seven entry points (crtfx_unpack.h), one more option.
 *
 * Status codes (crtfx_status), pixel formats (crtfx_pixfmt) and conventions are those of crtfx.h: the caller owns every frame; work is
 * enqueued on the caller's hipStream_t (void*, NULL = the default stream); only create / destroy synchronise; the calling thread's current
 * device must be the plan's when it runs.
 *
 * Layouts (crtfx_sited_layout), with cw = (w + 1) / 2 and ch = (h + 1) / 2, every row unpadded:
 *     yuv420p, nv12                 the geometry of crtfx_unpack.h      frame_bytes = h * w + 2 * ch * cw             uint8 h x w x 3 out
 *     yuv422p, yuyv422, uyvy422     the geometry of crtfx_422.h         h * w + 2 * h * cw (planar), 4 * h * cw       uint8 h x w x 3 out
 *                                   (the pad byte of an odd-width packed row is ignored)
 *     yuv420p10le, p010le           the geometry of crtfx_deep.h        2 * (h * w + 2 * ch * cw)                     half h x w x 3 out
 *                                   sample = word & 1023 / word >> 6, the other bits ignored; quarter codes q, out = half(q / 4)
 * The RGB pixel format follows from the layout: CRTFX_PIX_U8 for the five 8-bit layouts, CRTFX_PIX_F16 for the two 10-bit ones.
 *
 * Arithmetic.  Exact integers, one shift, one clamp.  C is a chroma plane of rows x cw samples, rows = ch (4:2:0) or h (4:2:2).  For the
 * luma pixel (x, y) the taps and their weights, in quarters:
 *     horizontal, siting left     the sample cx sits on luma column 2 cx (MPEG-2 / H.264 / HEVC).  cx = x >> 1;
 *                                 even x: (hn, hf) = (4, 0); odd x: (2, 2) with cxf = min(cx + 1, cw - 1)
 *     horizontal, siting center   the sample sits between columns 2 cx and 2 cx + 1 (JPEG / MPEG-1; the inverse siting of the egress stages'
 *                                 box mean).  (hn, hf) = (3, 1); even x: cxf = max(cx - 1, 0); odd x: cxf = min(cx + 1, cw - 1)
 *     vertical, 4:2:0             both sitings: chroma midway between two luma rows.  cy = y >> 1, (vn, vf) = (3, 1);
 *                                 even y: cyf = max(cy - 1, 0); odd y: cyf = min(cy + 1, rows - 1)
 *     vertical, 4:2:2             cy = y, (vn, vf) = (4, 0)
 *     D(C)   = vn * (hn * C[cy][cx] + hf * C[cy][cxf]) + vf * (hn * C[cyf][cx] + hf * C[cyf][cxf])                 weights sum to 16
 *     acc[k] = 16 * m[k][0] * (Y[y][x] - off0) + m[k][1] * (D(U) - 16 * off1) + m[k][2] * (D(V) - 16 * off2) + (1 << 19)      k = R, G, B
 *     8-bit:   out[k] = clamp(acc[k] >> 20, 0, 255)
 *     10-bit:  q[k] = clamp(acc[k] >> 20, 0, 1020),  out[k] = half(q[k] / 4)                                         exact: no rounding occurs
 * Edge taps are clamped indices: nothing outside the planes is read.  Where the taps of a pixel are equal the result is the replicating
 * stage's: acc = 16 * (its accumulator without the rounding term) + 2^19, the same floor after the shift.  So a frame with constant chroma
 * planes, a 1 x 1 and a 2 x 2 frame convert to the bytes of crtfx_unpack_* / crtfx_unpack422_* / crtfx_unpack10_*.  m and off are those
 * stages' (pythoncrt_amd.tables.rgb_matrix, rgb_matrix10).  NOT claimed: byte equality with libswscale.  What the tests hold the kernels to
 * is the arithmetic above (tests/sited_model.py).
 *
 * Accumulator width and the matrices create admits (every row k; CRTFX_E_INVALID otherwise):
 *     8-bit    (|m[k][0]| + |m[k][1]| + |m[k][2]|) * 255 * 16 + 2^19 < 2^31: acc stays in int32 for every input and every offset.
 *     10-bit   the sum does not fit (bt601 limited range, B row: about 2.3e9).  With A_i = max(off_i, 1023 - off_i), the largest magnitude of
 *              a centred sample: 16 * |m[k][0]| * A_0 < 2^31 and 16 * (|m[k][1]| * A_1 + |m[k][2]| * A_2) + 2^19 < 2^31.  The luma part and
 *              the chroma part (with the rounding term) then each fit int32; the kernels add them with a saturating 32-bit add.  A sum
 *              that saturates lies outside [0, 1020 << 20], where the clamp gives the same code as the exact sum, so the result is the
 *              int64 model's for every admitted matrix.
 *
 * Paths, chosen per run and named by crtfx_sited_last_plan; both give the same bytes.  Fourteen kernels, k_unpack_sited<layout, path>; the
 * siting travels as the four horizontal weights in the kernel arguments.
 *     vec       taken when w % 8 == 0 and the frame bases are 4-byte aligned: src_base and dst_base are multiples of 4, and with n > 1 so
 *               are both strides (the other stages' rule).  One lane owns 8 columns of two rows (4:2:0) or one row (4:2:2): its luma, its
 *               four chroma samples per plane and chroma row, and its RGB are dword-multiple accesses.  Consecutive lanes take consecutive
 *               column blocks; all n frames are one grid.  4:2:0 lanes read three chroma rows: above, own, below, clamped at the frame
 *               edges.  The chroma sample to the left and to the right of the lane's four is read with ONE NARROW LOAD each per chroma row
 *               and plane (a byte, a 16-bit word, or the neighbour's dword for nv12 / p010le pairs and packed macropixels), at a clamped
 *               index: a row end and a frame edge read the lane's own edge sample again, a wave end needs no special case.  The
 *               alternative — the neighbour lane's edge sample through a cross-lane move — saves those loads (they hit lines the
 *               neighbour lane fetches anyway) at the price of three exceptions (wave ends, row ends, frame edges) that need the narrow
 *               load regardless; it was not built.  An odd h is served: the last lane row of a 4:2:0 frame stores one row.
 *     general   any size and alignment (10-bit: even bases and strides): one lane per chroma sample and the up to 2 x 2 (4:2:0) or 2 x 1
 *               (4:2:2) pixels under it, byte loads and stores (10-bit: 16-bit ones); 3 x 3 (4:2:0) or 1 x 3 (4:2:2) chroma taps per plane
 *               at clamped indices.  Every output element is written by exactly one lane and nothing beyond x < w, y < h is read or
 *               written at an odd edge.  Also the A/B and test fallback (CRTFX_SITED_OPT_FORCE_GENERAL).
 * Registers (gfx950, as built; tests/test_sited_tables.py reads them from the library and holds every build to 128): VGPRs of
 * <layout>: vec / general —
 *     yuv420p 61 / 39     nv12 60 / 27     yuv422p 34 / 22     yuyv422 33 / 17     uyvy422 33 / 17     yuv420p10le 66 / 36     p010le 64 / 27
 * The 4:2:0 vec builds hold three chroma rows of six samples per plane beside two luma rows; only the yuv420p10le one passes 64 (seven
 * waves per SIMD instead of eight);
 * no AGPRs, no LDS, no scratch, no spills.
 * Measured once on one MI355X at 4K, batches of 8 frames (profiles/sited_chroma.txt, tools/sited_kernel_times.py): the vec builds take 10.3 -
 * 11.2 us per frame for the 8-bit layouts and 21.4 - 23.7 us for the 10-bit ones, 1.33 - 1.52 x the replicating stages' vec builds and 1.32 - 1.63 x
 * a device-to-device copy of the same traffic, and every vec build is 1.2 - 2.1 x faster than its general build (also at 1080p): "vec whenever
 * its conditions hold" stands.  The narrow-load form above is the one that was built and measured; the cross-lane form was not.
 */
#ifndef CRTFX_SITED_H
#define CRTFX_SITED_H

#include <stddef.h>
#include <stdint.h>

#include "crtfx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crtfx_sited crtfx_sited;

typedef enum crtfx_sited_layout {
    CRTFX_SITED_YUV420P = 0, CRTFX_SITED_NV12 = 1, CRTFX_SITED_YUV422P = 2, CRTFX_SITED_YUYV422 = 3, CRTFX_SITED_UYVY422 = 4,
    CRTFX_SITED_YUV420P10LE = 5, CRTFX_SITED_P010LE = 6
} crtfx_sited_layout;

typedef enum crtfx_sited_siting { CRTFX_SITED_LEFT = 0, CRTFX_SITED_CENTER = 1 } crtfx_sited_siting;

/* Plans the conversion on `device` (synchronises; the calling thread's current device is restored).  pix_fmt, the format of the RGB frames
 * written, must be the one the layout implies; the other one is CRTFX_E_UNSUPPORTED.  m: 9 integers (rows R, G, B over the columns Y, U, V),
 * off: 3 integers in 0..255 (8-bit layouts) or 0..1023 (10-bit).  CRTFX_E_INVALID: a size < 1 or > 32767, an unknown layout or pixel format,
 * a null table, an offset outside its range, or a matrix the rules above do not admit.  All of these are refused before a device is
 * touched.  When it fails *out_plan is NULL and crtfx_sited_last_error(NULL) holds the message (per calling thread).  The siting of a new
 * plan is CRTFX_SITED_LEFT. */
int crtfx_sited_create(int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, crtfx_sited** out_plan);
int crtfx_sited_destroy(crtfx_sited* plan);
const char* crtfx_sited_last_error(const crtfx_sited* plan);

/* The bytes of one SOURCE frame (the layout's expression above); 0 for a null plan. */
size_t crtfx_sited_frame_bytes(const crtfx_sited* plan);

/* n frames in one call: frame i is read at src_base + i * src_stride_bytes (frame_bytes bytes) and written at
 * dst_base + i * dst_stride_bytes (h x w x 3 bytes or halves, rows unpadded); strides of at least a frame.  The 8-bit layouts take any
 * byte base and stride; the 10-bit ones need even bases and strides (CRTFX_E_INVALID otherwise).  Bytes between frames are neither read
 * nor written.  Source and destination must not overlap. */
int crtfx_sited_run(crtfx_sited* plan, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream);

/* FORCE_GENERAL (0 / 1): take the narrow-access kernel whatever the width and alignment.  SITING (CRTFX_SITED_LEFT / CRTFX_SITED_CENTER):
 * the horizontal siting of the runs that follow; a live plan may be switched back and forth.  Any other option or value: CRTFX_E_INVALID. */
typedef enum crtfx_sited_option { CRTFX_SITED_OPT_FORCE_GENERAL = 1, CRTFX_SITED_OPT_SITING = 2 } crtfx_sited_option;
int crtfx_sited_set_option(crtfx_sited* plan, int option, int value);

/* The path of the most recent crtfx_sited_run (before the first one: the path a run with aligned bases would take) and the siting:
 * `sited=k_unpack_sited<nv12,vec>;siting=left;frames=5` or `sited=k_unpack_sited<p010le,general>;siting=center;frames=5`. */
int crtfx_sited_last_plan(crtfx_sited* plan, char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* CRTFX_SITED_H */
