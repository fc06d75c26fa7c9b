// crtfx_deint.hip — the deinterlace stage (include/crtfx_deint.h): two fields woven into one h x w x 3 frame become one or two progressive
// frames.  A vec and a general kernel per (method, sample type, field mode), the host glue, the C entry points.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <type_traits>

#include "crtfx_deint.h"
#include "crtfx_edge.hip.h"
#include "crtfx_frame_host.h"

namespace crtfx_deint_impl {

struct linear { static constexpr const char* name = "linear"; };
struct edge { static constexpr const char* name = "edge"; };

// Launch constants.
struct Args {
    const uint8_t* src;
    uint8_t* dst;
    size_t src_stride, dst_stride;      // bytes; the destination's is per OUTPUT frame
    uint32_t h, w;
    uint32_t blocks_row;                // vec: 8-pixel blocks per row (w / 8)
    uint32_t lanes;                     // vec: lanes per source frame (h * blocks_row)
    uint32_t first;                     // the field of output frame 0: 0 under TFF, 1 under BFF
};

// vec: one lane per 1 row x 8 pixels of the SOURCE frame: that block of every output frame is this lane's
template <class M, class P, class F>
__device__ __forceinline__ void deint_vec(const Args& a) {
    constexpr int SZ = sizeof(typename P::T), SPD = 4 / SZ;            // bytes per sample, samples per dword
    constexpr int CD = 24 / SPD, HD = 12 / SPD;                         // dwords of a block's 24 samples, and of the 4 pixels beside it
    constexpr uint32_t MASK = SZ == 1 ? 0xffu : 0xffffu;
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.lanes) return;
    const uint32_t y = i / a.blocks_row, bx = i - y * a.blocks_row;
    const size_t row = (size_t)a.w * 3u * SZ, col = (size_t)bx * 24u * SZ;
    const uint8_t* __restrict__ s = a.src + (size_t)blockIdx.z * a.src_stride;
    const uint32_t kept = ((y & 1u) == a.first) ? 1u : 0u;              // row y is kept in output frame 0 (the first field's) and made in frame 1, or the reverse
    uint8_t* __restrict__ dk;                                           // where row y is kept
    uint8_t* __restrict__ dm;                                           // where row y is made
    if constexpr (std::is_same<F, both>::value) {
        dk = a.dst + ((size_t)blockIdx.z * 2u + (1u - kept)) * a.dst_stride + (size_t)y * row + col;
        dm = a.dst + ((size_t)blockIdx.z * 2u + kept) * a.dst_stride + (size_t)y * row + col;
    } else {
        dk = dm = a.dst + (size_t)blockIdx.z * a.dst_stride + (size_t)y * row + col;
    }
    if (std::is_same<F, both>::value || kept) {                        // kept: the source's bits
        uint32_t c[CD];
        load_dwords<CD>(s + (size_t)y * row + col, c);
        store_dwords<CD>(dk, c);
    }
    if (!std::is_same<F, both>::value && kept) return;
    const bool two = y > 0u && y + 1u < a.h;                            // h >= 2: at least one neighbour row is in the frame
    const uint8_t* __restrict__ ra = s + (size_t)(y > 0u ? y - 1u : y + 1u) * row + col;
    const uint8_t* __restrict__ rb = s + (size_t)(y + 1u < a.h ? y + 1u : y - 1u) * row + col;
    uint32_t out[CD];
    if (!std::is_same<M, edge>::value || !two) {                        // LINEAR, and a row with one neighbour (a == b)
        uint32_t ca[CD], cb[CD];
        load_dwords<CD>(ra, ca);
        if (two) load_dwords<CD>(rb, cb);
#pragma unroll
        for (int k = 0; k < CD; ++k) {
            if (!two) cb[k] = ca[k];
            if constexpr (SZ == 1) {
                out[k] = (ca[k] | cb[k]) - (((ca[k] ^ cb[k]) >> 1) & 0x7f7f7f7fu);     // (a + b + 1) >> 1 in each byte
            } else {
                const int lo = (P::code(ca[k] & MASK) + P::code(cb[k] & MASK) + 1) >> 1, hi = (P::code(ca[k] >> 16) + P::code(cb[k] >> 16) + 1) >> 1;
                out[k] = P::bits(lo) | P::bits(hi) << 16;
            }
        }
    } else {
        // the 16 pixels x0 - 4 .. x0 + 11 of both rows: the block and the four pixels on either side, which are blocks of the same row.  A
        // block at a row's end has no such side; its slots stay zero and only pixels that take d = 0 would have looked at them.
        uint32_t wa[CD + 2 * HD] = {}, wb[CD + 2 * HD] = {};
        load_dwords<CD>(ra, wa + HD);
        load_dwords<CD>(rb, wb + HD);
        if (bx > 0u) { load_dwords<HD>(ra - 4 * HD, wa); load_dwords<HD>(rb - 4 * HD, wb); }
        if (bx + 1u < a.blocks_row) { load_dwords<HD>(ra + 4 * CD, wa + HD + CD); load_dwords<HD>(rb + 4 * CD, wb + HD + CD); }
        int A[8 + 2 * REACH][3], B[8 + 2 * REACH][3];                   // window index i <-> pixel x0 - 3 + i: sample 3 (i + 1) + k of the 48 loaded
#pragma unroll
        for (int p = 0; p < 8 + 2 * REACH; ++p)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int sidx = 3 * (p + 1) + k;
                A[p][k] = P::code((wa[sidx / SPD] >> (8 * SZ * (sidx % SPD))) & MASK);
                B[p][k] = P::code((wb[sidx / SPD] >> (8 * SZ * (sidx % SPD))) & MASK);
            }
        int d[8];
        edge_search<8>(A, B, d);
        const uint32_t x0 = bx * 8u;
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
                const int sidx = 3 * p + k;
                out[sidx / SPD] |= P::bits((va + vb + 1) >> 1) << (8 * SZ * (sidx % SPD));
            }
        }
    }
    store_dwords<CD>(dm, out);
}

// general: one lane per pixel of the SOURCE frame: that pixel of every output frame is this lane's
template <class M, class P, class F>
__device__ __forceinline__ void deint_general(const Args& a) {
    typedef typename P::T T;
    const uint32_t x = blockIdx.x * BLOCK + threadIdx.x, y = blockIdx.y;
    if (x >= a.w) return;
    const size_t row = (size_t)a.w * 3u, o = (size_t)y * row + (size_t)x * 3u;
    const T* __restrict__ s = reinterpret_cast<const T*>(a.src + (size_t)blockIdx.z * a.src_stride);
    const uint32_t kept = ((y & 1u) == a.first) ? 1u : 0u;
    T* __restrict__ dk;
    T* __restrict__ dm;
    if constexpr (std::is_same<F, both>::value) {
        dk = reinterpret_cast<T*>(a.dst + ((size_t)blockIdx.z * 2u + (1u - kept)) * a.dst_stride);
        dm = reinterpret_cast<T*>(a.dst + ((size_t)blockIdx.z * 2u + kept) * a.dst_stride);
    } else {
        dk = dm = reinterpret_cast<T*>(a.dst + (size_t)blockIdx.z * a.dst_stride);
    }
    if (std::is_same<F, both>::value || kept) {
#pragma unroll
        for (int k = 0; k < 3; ++k) dk[o + k] = s[o + k];
    }
    if (!std::is_same<F, both>::value && kept) return;
    const bool two = y > 0u && y + 1u < a.h;
    const T* __restrict__ ra = s + (size_t)(y > 0u ? y - 1u : y + 1u) * row;
    const T* __restrict__ rb = s + (size_t)(y + 1u < a.h ? y + 1u : y - 1u) * row;
    int dd = 0;
    if constexpr (std::is_same<M, edge>::value) {
        if (two && x >= (uint32_t)REACH && x + REACH < a.w) {           // columns x - 3 .. x + 3 are in the row
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
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)                                         // |dd| <= 2 < REACH: inside the row
        dm[o + k] = (T)P::bits((P::code(ra[(size_t)((int)x + dd) * 3u + k]) + P::code(rb[(size_t)((int)x - dd) * 3u + k]) + 1) >> 1);
}

template <class M, class P, class F, class Path>
__global__ __launch_bounds__(BLOCK) void k_deint(Args a) {
    if constexpr (std::is_same<Path, vec>::value) deint_vec<M, P, F>(a); else deint_general<M, P, F>(a);
}

}  // namespace crtfx_deint_impl

using namespace crtfx_deint_impl;

struct crtfx_deint : crtfx_frames::Plan {      // one frame size and sample type on both sides; frames_out = 2 under fields=both
    int h = 0, w = 0;
    bool half = false, edge = false, bff = false, both = false;
};

namespace {

using crtfx_frames::Batch;
using crtfx_stage::create_err;
using crtfx_stage::fail;

template <class M, class P, class F>
void launch_path(bool fits, dim3 grid, hipStream_t st, const Args& a) {
    if (fits) hipLaunchKernelGGL((k_deint<M, P, F, vec>), grid, dim3(BLOCK), 0, st, a);
    else hipLaunchKernelGGL((k_deint<M, P, F, general>), grid, dim3(BLOCK), 0, st, a);
}

template <class M, class P>
void launch_fields(const crtfx_deint* p, bool fits, dim3 grid, hipStream_t st, const Args& a) {
    if (p->both) launch_path<M, P, both>(fits, grid, st, a); else launch_path<M, P, first>(fits, grid, st, a);
}

template <class M>
void launch_pix(const crtfx_deint* p, bool fits, dim3 grid, hipStream_t st, const Args& a) {
    if (p->half) launch_fields<M, f16>(p, fits, grid, st, a); else launch_fields<M, u8>(p, fits, grid, st, a);
}

struct U : crtfx_frames::Unit {
    using H = crtfx_deint;
    static constexpr int force_option = CRTFX_DEINT_OPT_FORCE_GENERAL;
    static constexpr const char* name = "deint";
    static constexpr bool one_size = true;

    // the vec kernels' conditions (crtfx_deint.h); b.n counts source frames
    static bool vec_fits(const H* p, const Batch& b) {
        if (p->force_general || (p->w & 7)) return false;
        if ((reinterpret_cast<uintptr_t>(b.src) | reinterpret_cast<uintptr_t>(b.dst)) & 3u) return false;
        if (b.n > 1 && (b.src_stride & 3u)) return false;
        return (size_t)b.n * p->frames_out <= 1 || !(b.dst_stride & 3u);
    }

    static void note_plan(H* p, bool fits, int frames) {
        snprintf(p->plan, sizeof p->plan, "deint=k_deint<%s,%s,%s,%s>;frames=%d", p->edge ? edge::name : linear::name, p->half ? f16::name : u8::name,
                 p->both ? both::name : first::name, fits ? vec::name : general::name, frames);
    }

    static Args make_args(const H* p, bool, const Batch&) {
        Args a{};
        a.h = (uint32_t)p->h; a.w = (uint32_t)p->w;
        a.blocks_row = a.w / 8u;
        a.lanes = a.h * a.blocks_row;                                   // below 2^27
        a.first = p->bff ? 1u : 0u;
        return a;
    }

    static void launch(const H* p, bool fits, Args& a, int, unsigned g, hipStream_t st) {
        const dim3 grid = fits ? dim3((a.lanes + BLOCK - 1) / BLOCK, 1, g) : dim3((a.w + BLOCK - 1) / BLOCK, p->h, g);
        if (p->edge) launch_pix<edge>(p, fits, grid, st, a); else launch_pix<linear>(p, fits, grid, st, a);
    }
};

}  // namespace

extern "C" {

const char* crtfx_deint_last_error(const crtfx_deint* p) { return p ? p->err.c_str() : create_err<crtfx_deint>().c_str(); }

int crtfx_deint_create(int device, int h, int w, int pix_fmt, int method, int order, int fields, crtfx_deint** out_plan) {
    using H = crtfx_deint;
    if (const int rc = crtfx_frames::begin_create(out_plan)) return rc;
    if (h < 2 || h > 32767) return fail<H>(nullptr, CRTFX_E_INVALID, "h = %d outside 2..32767 (a frame of two fields has two rows)", h);
    if (const int rc = crtfx_frames::check_size<H>("w", w)) return rc;
    if (pix_fmt != CRTFX_PIX_U8 && pix_fmt != CRTFX_PIX_F16) return fail<H>(nullptr, CRTFX_E_INVALID, "unknown pix_fmt %d", pix_fmt);
    if (method != CRTFX_DEINT_LINEAR && method != CRTFX_DEINT_EDGE) return fail<H>(nullptr, CRTFX_E_INVALID, "unknown method %d", method);
    if (order != CRTFX_DEINT_TFF && order != CRTFX_DEINT_BFF) return fail<H>(nullptr, CRTFX_E_INVALID, "unknown order %d", order);
    if (fields != CRTFX_DEINT_FIRST && fields != CRTFX_DEINT_BOTH) return fail<H>(nullptr, CRTFX_E_INVALID, "unknown fields %d", fields);
    return crtfx_frames::new_plan<U>(device, out_plan, [&](H* p) {
        p->h = h; p->w = w;
        p->half = pix_fmt == CRTFX_PIX_F16; p->edge = method == CRTFX_DEINT_EDGE; p->bff = order == CRTFX_DEINT_BFF; p->both = fields == CRTFX_DEINT_BOTH;
        p->src_bps = p->dst_bps = p->half ? 2 : 1;
        p->src_bytes = p->dst_bytes = (size_t)h * w * 3 * p->src_bps;
        p->frames_out = p->both ? 2 : 1;
        return CRTFX_OK;
    });
}

int crtfx_deint_frames_out(const crtfx_deint* p) { return p ? p->frames_out : 0; }

int crtfx_deint_destroy(crtfx_deint* p) { return crtfx_frames::destroy(p); }

int crtfx_deint_set_option(crtfx_deint* p, int option, int value) { return crtfx_frames::set_option<U>(p, option, value); }

int crtfx_deint_last_plan(crtfx_deint* p, char* buf, size_t n) { return crtfx_frames::last_plan(p, buf, n); }

int crtfx_deint_run(crtfx_deint* p, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream) {
    return crtfx_frames::run<U>(p, Batch{nullptr, src_base, src_stride_bytes, dst_base, dst_stride_bytes, n}, stream);
}

}  // extern "C"

