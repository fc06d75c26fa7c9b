// crtfx_adeint.hip — the motion-adaptive deinterlace stage (include/crtfx_adeint.h): per made sample EDGE's interpolation, clamped to within
// m of the source's own sample, m being what the picture changed by since the previous frame.  A vec and a general kernel per (sample type,
// field mode), the host glue, the C entry points.  The direction search, the sample types and the dword helpers are crtfx_deint.hip's
// (crtfx_edge.hip.h).

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <type_traits>

#include "crtfx_adeint.h"
#include "crtfx_edge.hip.h"
#include "crtfx_frame_host.h"

namespace crtfx_adeint_impl {

using namespace crtfx_deint_impl;       // the tags, u8 / f16, load_dwords / store_dwords, edge_search, BLOCK, REACH

// Launch constants.
struct Args {
    const uint8_t* src;
    const uint8_t* prev;                // the previous frame of source frame 0 of this launch, or null: that frame has none
    uint8_t* dst;
    size_t src_stride, dst_stride;      // bytes; the destination's is per OUTPUT frame
    uint32_t h, w;
    uint32_t blocks_row;                // vec: 8-pixel blocks per row (w / 8)
    uint32_t lanes;                     // vec: lanes per source frame (h * blocks_row)
    uint32_t first;                     // the field of output frame 0: 0 under TFF, 1 under BFF
};

constexpr int NO_P = 1 << 20;           // m without a previous frame: past every |e - c|, so the clamp leaves e

__device__ __forceinline__ int absdiff(int a, int b) { const int t = a - b; return t < 0 ? -t : t; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }

// vec: one lane per 1 row x 8 pixels of the SOURCE frame: that block of every output frame is this lane's
template <class P, class F>
__device__ __forceinline__ void adeint_vec(const Args& a) {
    constexpr int SZ = sizeof(typename P::T), SPD = 4 / SZ;            // bytes per sample, samples per dword
    constexpr int CD = 24 / SPD, HD = 12 / SPD;                         // dwords of a block's 24 samples, and of the 4 pixels beside it
    static_assert(SPD == P::SPD, "samples per dword");
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.lanes) return;
    const uint32_t y = i / a.blocks_row, bx = i - y * a.blocks_row;
    const size_t row = (size_t)a.w * 3u * SZ, col = (size_t)bx * 24u * SZ;
    const uint8_t* __restrict__ s = a.src + (size_t)blockIdx.z * a.src_stride;
    const uint8_t* __restrict__ pv = blockIdx.z ? s - a.src_stride : a.prev;       // P: the frame before C in the batch, or the caller's
    const uint32_t kept = ((y & 1u) == a.first) ? 1u : 0u;              // row y is kept in output frame 0 (the first field's) and made in frame 1, or the reverse
    uint8_t* __restrict__ dk;                                           // where row y is kept
    uint8_t* __restrict__ dm;                                           // where row y is made
    if constexpr (std::is_same<F, both>::value) {
        dk = a.dst + ((size_t)blockIdx.z * 2u + (1u - kept)) * a.dst_stride + (size_t)y * row + col;
        dm = a.dst + ((size_t)blockIdx.z * 2u + kept) * a.dst_stride + (size_t)y * row + col;
    } else {
        dk = dm = a.dst + (size_t)blockIdx.z * a.dst_stride + (size_t)y * row + col;
    }
    uint32_t cy[CD];                                                    // C's row y: the kept bits, and the centre of the made samples' clamp
    load_dwords<CD>(s + (size_t)y * row + col, cy);
    if (std::is_same<F, both>::value || kept) store_dwords<CD>(dk, cy);
    if (!std::is_same<F, both>::value && kept) return;
    const bool two = y > 0u && y + 1u < a.h;                            // h >= 2: at least one neighbour row is in the frame
    const size_t oa = (size_t)(y > 0u ? y - 1u : y + 1u) * row + col, ob = (size_t)(y + 1u < a.h ? y + 1u : y - 1u) * row + col;
    const uint8_t* __restrict__ ra = s + oa;
    const uint8_t* __restrict__ rb = s + ob;
    // the 16 pixels x0 - 4 .. x0 + 11 of both rows, as k_deint<edge,...,vec> loads them: the block and, for a row with two neighbours, the four
    // pixels on either side where the row has them.  With one neighbour a == b, d = 0 and (a + a + 1) >> 1 = a: the copy of that row.
    uint32_t wa[CD + 2 * HD] = {}, wb[CD + 2 * HD] = {};
    load_dwords<CD>(ra, wa + HD);
    load_dwords<CD>(rb, wb + HD);
    if (two && bx > 0u) { load_dwords<HD>(ra - 4 * HD, wa); load_dwords<HD>(rb - 4 * HD, wb); }
    if (two && bx + 1u < a.blocks_row) { load_dwords<HD>(ra + 4 * CD, wa + HD + CD); load_dwords<HD>(rb + 4 * CD, wb + HD + CD); }
    int A[8 + 2 * REACH][3], B[8 + 2 * REACH][3];                       // window index i <-> pixel x0 - 3 + i: sample 3 (i + 1) + k of the 48 loaded
    {
        int qa[48], qb[48];                                             // a dword's samples are converted together (P::codes)
        unpack_codes<P, CD + 2 * HD>(wa, qa);
        unpack_codes<P, CD + 2 * HD>(wb, qb);
#pragma unroll
        for (int p = 0; p < 8 + 2 * REACH; ++p)
#pragma unroll
            for (int k = 0; k < 3; ++k) { A[p][k] = qa[3 * (p + 1) + k]; B[p][k] = qb[3 * (p + 1) + k]; }
    }
    // m per pixel from the lane's own block of P's rows y - 1, y, y + 1: no halo, m is per pixel
    int c[8][3], m[8];
    {
        int qc[24];
        unpack_codes<P, CD>(cy, qc);
#pragma unroll
        for (int p = 0; p < 8; ++p)
#pragma unroll
            for (int k = 0; k < 3; ++k) c[p][k] = qc[3 * p + k];
    }
    if (pv) {
        uint32_t py[CD], pa[CD], pb[CD];
        load_dwords<CD>(pv + (size_t)y * row + col, py);
        load_dwords<CD>(pv + oa, pa);
        load_dwords<CD>(pv + ob, pb);
        int qy[24], qa[24], qb[24];
        unpack_codes<P, CD>(py, qy);
        unpack_codes<P, CD>(pa, qa);
        unpack_codes<P, CD>(pb, qb);
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            int mm = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int t0 = absdiff(c[p][k], qy[3 * p + k]);
                const int t1 = (absdiff(A[p + REACH][k], qa[3 * p + k]) + absdiff(B[p + REACH][k], qb[3 * p + k]) + 1) >> 1;
                mm = imax(mm, imax(t0, t1));
            }
            m[p] = mm;
        }
    } else {
#pragma unroll
        for (int p = 0; p < 8; ++p) m[p] = NO_P;
    }
    int d[8] = {};
    if (two) edge_search<8>(A, B, d);
    const uint32_t x0 = bx * 8u;
    uint32_t out[CD];
#pragma unroll
    for (int k = 0; k < CD; ++k) out[k] = 0u;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const int dd = (x0 + p >= (uint32_t)REACH && x0 + p + REACH < a.w) ? d[p] : 0;      // x < 3 or x > w - 4: d = 0
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            int va = A[p + REACH][k], vb = B[p + REACH][k];
#pragma unroll
            for (int j = -2; j <= 2; ++j) {
                if (j == 0) continue;
                va = dd == j ? A[p + REACH + j][k] : va;
                vb = dd == j ? B[p + REACH - j][k] : vb;
            }
            const int e = (va + vb + 1) >> 1;
            const int r = imin(imax(e, c[p][k] - m[p]), c[p][k] + m[p]);       // between e and c: a code
            const int sidx = 3 * p + k;
            out[sidx / SPD] |= P::bits(r) << (8 * SZ * (sidx % SPD));
        }
    }
    store_dwords<CD>(dm, out);
}

// general: one lane per pixel of the SOURCE frame: that pixel of every output frame is this lane's
template <class P, class F>
__device__ __forceinline__ void adeint_general(const Args& a) {
    typedef typename P::T T;
    const uint32_t x = blockIdx.x * BLOCK + threadIdx.x, y = blockIdx.y;
    if (x >= a.w) return;
    const size_t row = (size_t)a.w * 3u, o = (size_t)y * row + (size_t)x * 3u;
    const uint8_t* sb = a.src + (size_t)blockIdx.z * a.src_stride;
    const T* __restrict__ s = reinterpret_cast<const T*>(sb);
    const T* __restrict__ pv = reinterpret_cast<const T*>(blockIdx.z ? sb - a.src_stride : a.prev);
    const uint32_t kept = ((y & 1u) == a.first) ? 1u : 0u;
    T* __restrict__ dk;
    T* __restrict__ dm;
    if constexpr (std::is_same<F, both>::value) {
        dk = reinterpret_cast<T*>(a.dst + ((size_t)blockIdx.z * 2u + (1u - kept)) * a.dst_stride);
        dm = reinterpret_cast<T*>(a.dst + ((size_t)blockIdx.z * 2u + kept) * a.dst_stride);
    } else {
        dk = dm = reinterpret_cast<T*>(a.dst + (size_t)blockIdx.z * a.dst_stride);
    }
    T cy[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) cy[k] = s[o + k];
    if (std::is_same<F, both>::value || kept) {
#pragma unroll
        for (int k = 0; k < 3; ++k) dk[o + k] = cy[k];
    }
    if (!std::is_same<F, both>::value && kept) return;
    const bool two = y > 0u && y + 1u < a.h;
    const size_t oa = (size_t)(y > 0u ? y - 1u : y + 1u) * row, ob = (size_t)(y + 1u < a.h ? y + 1u : y - 1u) * row;
    const T* __restrict__ ra = s + oa;
    const T* __restrict__ rb = s + ob;
    int m = NO_P;
    if (pv) {
        m = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int t0 = absdiff(P::code(cy[k]), P::code(pv[o + k]));
            const int t1 = (absdiff(P::code(ra[(size_t)x * 3u + k]), P::code(pv[oa + (size_t)x * 3u + k])) +
                            absdiff(P::code(rb[(size_t)x * 3u + k]), P::code(pv[ob + (size_t)x * 3u + k])) + 1) >> 1;
            m = imax(m, imax(t0, t1));
        }
    }
    int dd = 0;
    if (two && x >= (uint32_t)REACH && x + REACH < a.w) {               // columns x - 3 .. x + 3 are in the row
        int A[1 + 2 * REACH][3], B[1 + 2 * REACH][3], d[1];
#pragma unroll
        for (int p = 0; p < 1 + 2 * REACH; ++p)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                A[p][k] = P::code(ra[(size_t)(x - REACH + p) * 3u + k]);
                B[p][k] = P::code(rb[(size_t)(x - REACH + p) * 3u + k]);
            }
        edge_search<1>(A, B, d);
        dd = d[0];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {                                       // |dd| <= 2 < REACH: inside the row
        const int e = (P::code(ra[(size_t)((int)x + dd) * 3u + k]) + P::code(rb[(size_t)((int)x - dd) * 3u + k]) + 1) >> 1;
        const int cc = P::code(cy[k]);
        dm[o + k] = (T)P::bits(imin(imax(e, cc - m), cc + m));
    }
}

template <class P, class F, class Path>
__global__ __launch_bounds__(BLOCK) void k_adeint(Args a) {
    if constexpr (std::is_same<Path, vec>::value) adeint_vec<P, F>(a); else adeint_general<P, F>(a);
}

}  // namespace crtfx_adeint_impl

using namespace crtfx_adeint_impl;

struct crtfx_adeint : crtfx_frames::Plan {     // one frame size and sample type on both sides; frames_out = 2 under fields=both
    int h = 0, w = 0;
    bool half = false, bff = false, both = false;
};

namespace {

using crtfx_frames::Batch;
using crtfx_stage::create_err;
using crtfx_stage::fail;

template <class P, class F>
void launch_path(bool fits, dim3 grid, hipStream_t st, const Args& a) {
    if (fits) hipLaunchKernelGGL((k_adeint<P, F, vec>), grid, dim3(BLOCK), 0, st, a);
    else hipLaunchKernelGGL((k_adeint<P, F, general>), grid, dim3(BLOCK), 0, st, a);
}

template <class P>
void launch_fields(const crtfx_adeint* p, bool fits, dim3 grid, hipStream_t st, const Args& a) {
    if (p->both) launch_path<P, both>(fits, grid, st, a); else launch_path<P, first>(fits, grid, st, a);
}

struct U : crtfx_frames::Unit {
    using H = crtfx_adeint;
    static constexpr int force_option = CRTFX_ADEINT_OPT_FORCE_GENERAL;
    static constexpr const char* name = "adeint";
    static constexpr bool one_size = true;

    // the vec kernels' conditions (crtfx_adeint.h); b.n counts source frames
    static bool vec_fits(const H* p, const Batch& b) {
        if (p->force_general || (p->w & 7)) return false;
        if ((reinterpret_cast<uintptr_t>(b.src) | reinterpret_cast<uintptr_t>(b.dst) | reinterpret_cast<uintptr_t>(b.prev)) & 3u) return false;
        if (b.n > 1 && (b.src_stride & 3u)) return false;
        return (size_t)b.n * p->frames_out <= 1 || !(b.dst_stride & 3u);
    }

    static void note_plan(H* p, bool fits, int frames) {
        snprintf(p->plan, sizeof p->plan, "adeint=k_adeint<%s,%s,%s>;frames=%d", p->half ? f16::name : u8::name, p->both ? both::name : first::name,
                 fits ? vec::name : general::name, frames);
    }

    static Args make_args(const H* p, bool, const Batch& b) {
        Args a{};
        a.prev = static_cast<const uint8_t*>(b.prev);
        a.h = (uint32_t)p->h; a.w = (uint32_t)p->w;
        a.blocks_row = a.w / 8u;
        a.lanes = a.h * a.blocks_row;                                   // below 2^27
        a.first = p->bff ? 1u : 0u;
        return a;
    }

    static void launch(const H* p, bool fits, Args& a, int f, unsigned g, hipStream_t st) {
        if (f) a.prev = a.src - a.src_stride;                           // a later group: the last frame of the group before it
        const dim3 grid = fits ? dim3((a.lanes + BLOCK - 1) / BLOCK, 1, g) : dim3((a.w + BLOCK - 1) / BLOCK, p->h, g);
        if (p->half) launch_fields<f16>(p, fits, grid, st, a); else launch_fields<u8>(p, fits, grid, st, a);
    }
};

}  // namespace

extern "C" {

const char* crtfx_adeint_last_error(const crtfx_adeint* p) { return p ? p->err.c_str() : create_err<crtfx_adeint>().c_str(); }

int crtfx_adeint_create(int device, int h, int w, int pix_fmt, int order, int fields, crtfx_adeint** out_plan) {
    using H = crtfx_adeint;
    if (const int rc = crtfx_frames::begin_create(out_plan)) return rc;
    if (h < 2 || h > 32767) return fail<H>(nullptr, CRTFX_E_INVALID, "h = %d outside 2..32767 (a frame of two fields has two rows)", h);
    if (const int rc = crtfx_frames::check_size<H>("w", w)) return rc;
    if (pix_fmt != CRTFX_PIX_U8 && pix_fmt != CRTFX_PIX_F16) return fail<H>(nullptr, CRTFX_E_INVALID, "unknown pix_fmt %d", pix_fmt);
    if (order != CRTFX_DEINT_TFF && order != CRTFX_DEINT_BFF) return fail<H>(nullptr, CRTFX_E_INVALID, "unknown order %d", order);
    if (fields != CRTFX_DEINT_FIRST && fields != CRTFX_DEINT_BOTH) return fail<H>(nullptr, CRTFX_E_INVALID, "unknown fields %d", fields);
    return crtfx_frames::new_plan<U>(device, out_plan, [&](H* p) {
        p->h = h; p->w = w;
        p->half = pix_fmt == CRTFX_PIX_F16; p->bff = order == CRTFX_DEINT_BFF; p->both = fields == CRTFX_DEINT_BOTH;
        p->src_bps = p->dst_bps = p->half ? 2 : 1;
        p->src_bytes = p->dst_bytes = (size_t)h * w * 3 * p->src_bps;
        p->frames_out = p->both ? 2 : 1;
        return CRTFX_OK;
    });
}

int crtfx_adeint_frames_out(const crtfx_adeint* p) { return p ? p->frames_out : 0; }

int crtfx_adeint_destroy(crtfx_adeint* p) { return crtfx_frames::destroy(p); }

int crtfx_adeint_set_option(crtfx_adeint* p, int option, int value) { return crtfx_frames::set_option<U>(p, option, value); }

int crtfx_adeint_last_plan(crtfx_adeint* p, char* buf, size_t n) { return crtfx_frames::last_plan(p, buf, n); }

int crtfx_adeint_run(crtfx_adeint* p, const void* prev_frame, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes,
                     int n, void* stream) {
    return crtfx_frames::run<U>(p, Batch{prev_frame, src_base, src_stride_bytes, dst_base, dst_stride_bytes, n}, stream);
}

}  // extern "C"

