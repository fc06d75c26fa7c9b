// crtfx_depth.hip — the depth stage (include/crtfx_depth.h): uint8 RGB frames widened to half, half frames narrowed to uint8 with plain
// rounding or ordered dither.  A vec and a general kernel per direction, the host glue, the C entry points.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <type_traits>

#include "crtfx_depth.h"
#include "crtfx_frame_host.h"

namespace crtfx_depth_impl {

struct none { static constexpr const char* name = "none"; };
struct ordered { static constexpr const char* name = "ordered"; };
struct vec {};
struct general {};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef u32x4 u32x4_dword_aligned __attribute__((aligned(4)));          // a 16-byte access at a dword-aligned address
typedef u32x2 u32x2_dword_aligned __attribute__((aligned(4)));          // an 8-byte one

// Launch constants.
struct Args {
    const uint8_t* src;
    uint8_t* dst;
    size_t src_stride, dst_stride;      // bytes
    uint32_t row;                       // samples per row (w * 3)
    uint32_t lanes_row;                 // narrow vec: lanes per row (w / 8)
    uint32_t len;                       // narrow vec: lanes per frame; widen vec: samples per frame (below 2^31); general: unused
};

constexpr int BLOCK = 256;

alignas(8) __constant__ uint8_t kBayer[64] = CRTFX_DEPTH_BAYER8;                      // a row is one 8-byte load

__device__ __forceinline__ float threshold(uint32_t b) { return (float)(2u * b + 1u) * (1.0f / 128.0f); }      // exact: an odd k < 128 over 2^7

template <class D>
__device__ __forceinline__ uint32_t narrow_one(uint32_t bits, float t) {
    const float f = (float)__builtin_bit_cast(_Float16, (uint16_t)bits);
    float v = f > 0.0f ? f : 0.0f;                                      // NaN, -0, negatives, -inf -> 0
    v = v < 255.0f ? v : 255.0f;                                        // +inf -> 255
    if constexpr (std::is_same<D, ordered>::value) return (uint32_t)(v + t);       // the sum is exact (crtfx_depth.h); truncation is the floor
    else return (uint32_t)rintf(v);                                     // ties to even
}

__device__ __forceinline__ uint32_t widen_one(uint32_t u) {
    return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)(float)u);
}

// vec: one lane per 1 row x 8 pixels: 24 halves in, 24 bytes out
template <class D>
__device__ __forceinline__ void narrow_vec(const Args& a) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.len) return;
    const uint8_t* __restrict__ s = a.src + (size_t)blockIdx.z * a.src_stride + (size_t)i * 48u;
    uint8_t* __restrict__ d = a.dst + (size_t)blockIdx.z * a.dst_stride + (size_t)i * 24u;
    const u32x4 q0 = reinterpret_cast<const u32x4_dword_aligned*>(s)[0];
    const u32x4 q1 = reinterpret_cast<const u32x4_dword_aligned*>(s)[1];
    const u32x4 q2 = reinterpret_cast<const u32x4_dword_aligned*>(s)[2];
    const uint32_t in[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
    float t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if constexpr (std::is_same<D, ordered>::value) {
        const uint32_t y = i / a.lanes_row;
        const u32x2 b = *reinterpret_cast<const u32x2*>(kBayer + 8u * (y & 7u));       // the lane's pixels are columns 8 k .. 8 k + 7: x & 7 = 0..7
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = threshold(((j < 4 ? b.x : b.y) >> (8 * (j & 3))) & 0xffu);
    }
    uint32_t out[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 24; ++k) {                                      // sample k of the lane: pixel k / 3
        const uint32_t bits = (k & 1) ? in[k >> 1] >> 16 : in[k >> 1] & 0xffffu;
        out[k >> 2] |= narrow_one<D>(bits, t[k / 3]) << (8 * (k & 3));
    }
    const u32x4 lo = {out[0], out[1], out[2], out[3]};
    const u32x2 hi = {out[4], out[5]};
    *reinterpret_cast<u32x4_dword_aligned*>(d) = lo;
    *reinterpret_cast<u32x2_dword_aligned*>(d + 16) = hi;
}

// general: one lane per sample
template <class D>
__device__ __forceinline__ void narrow_general(const Args& a) {
    const uint32_t xs = blockIdx.x * BLOCK + threadIdx.x, y = blockIdx.y;
    if (xs >= a.row) return;
    const uint16_t* __restrict__ s = reinterpret_cast<const uint16_t*>(a.src + (size_t)blockIdx.z * a.src_stride);
    uint8_t* __restrict__ d = a.dst + (size_t)blockIdx.z * a.dst_stride;
    const size_t o = (size_t)y * a.row + xs;
    float t = 0.0f;
    if constexpr (std::is_same<D, ordered>::value) t = threshold(kBayer[8u * (y & 7u) + ((xs / 3u) & 7u)]);
    d[o] = (uint8_t)narrow_one<D>(s[o], t);
}

// vec: one lane per chunk of 16 samples of the frame
__device__ __forceinline__ void widen_vec(const Args& a) {
    const uint32_t o = (blockIdx.x * BLOCK + threadIdx.x) * 16u;        // len < 2^31: no wrap
    if (o >= a.len) return;
    const uint8_t* __restrict__ s = a.src + (size_t)blockIdx.z * a.src_stride + o;
    uint8_t* __restrict__ d = a.dst + (size_t)blockIdx.z * a.dst_stride + (size_t)o * 2u;
    if (o + 16u <= a.len) {
        const u32x4 q = *reinterpret_cast<const u32x4_dword_aligned*>(s);
        const uint32_t in[4] = {q.x, q.y, q.z, q.w};
        uint32_t out[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {                                   // samples 2 k and 2 k + 1
            const uint32_t w = in[k >> 1] >> (16 * (k & 1));
            out[k] = widen_one(w & 0xffu) | widen_one((w >> 8) & 0xffu) << 16;
        }
        const u32x4 lo = {out[0], out[1], out[2], out[3]}, hi = {out[4], out[5], out[6], out[7]};
        reinterpret_cast<u32x4_dword_aligned*>(d)[0] = lo;
        reinterpret_cast<u32x4_dword_aligned*>(d)[1] = hi;
        return;
    }
    const uint32_t r = a.len - o;                                       // 1..15 samples: the frame's tail
    uint32_t k = 0;
#pragma unroll 1
    for (; k + 4u <= r; k += 4u) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(s + k);
        uint32_t* dd = reinterpret_cast<uint32_t*>(d + 2u * k);
        dd[0] = widen_one(w & 0xffu) | widen_one((w >> 8) & 0xffu) << 16;
        dd[1] = widen_one((w >> 16) & 0xffu) | widen_one(w >> 24) << 16;
    }
#pragma unroll 1
    for (; k < r; ++k) reinterpret_cast<uint16_t*>(d)[k] = (uint16_t)widen_one(s[k]);
}

__device__ __forceinline__ void widen_general(const Args& a) {
    const uint32_t xs = blockIdx.x * BLOCK + threadIdx.x, y = blockIdx.y;
    if (xs >= a.row) return;
    const uint8_t* __restrict__ s = a.src + (size_t)blockIdx.z * a.src_stride;
    uint16_t* __restrict__ d = reinterpret_cast<uint16_t*>(a.dst + (size_t)blockIdx.z * a.dst_stride);
    const size_t o = (size_t)y * a.row + xs;
    d[o] = (uint16_t)widen_one(s[o]);
}

template <class D, class Path>
__global__ __launch_bounds__(BLOCK) void k_narrow(Args a) {
    if constexpr (std::is_same<Path, vec>::value) narrow_vec<D>(a); else narrow_general<D>(a);
}

template <class Path>
__global__ __launch_bounds__(BLOCK) void k_widen(Args a) {
    if constexpr (std::is_same<Path, vec>::value) widen_vec(a); else widen_general(a);
}

}  // namespace crtfx_depth_impl

using namespace crtfx_depth_impl;

struct crtfx_depth : crtfx_frames::Plan {      // the side whose bps is 2 is the half side
    int h = 0, w = 0;
    bool narrow = false, dither = false;
    size_t samples = 0;                 // of one frame
};

namespace {

using crtfx_frames::Batch;
using crtfx_stage::create_err;
using crtfx_stage::fail;

struct U : crtfx_frames::Unit {
    using H = crtfx_depth;
    static constexpr int force_option = CRTFX_DEPTH_OPT_FORCE_GENERAL;
    static constexpr const char* name = "depth";

    // the vec kernels' conditions (crtfx_depth.h)
    static bool vec_fits(const H* p, const Batch& b) {
        if (p->force_general) return false;
        if (p->narrow ? (p->w & 7) != 0 : p->samples >= (1ull << 31)) return false;
        if ((reinterpret_cast<uintptr_t>(b.src) | reinterpret_cast<uintptr_t>(b.dst)) & 3u) return false;
        return b.n <= 1 || !((b.src_stride | b.dst_stride) & 3u);
    }

    static void note_plan(H* p, bool vec, int frames) {
        const char* path = vec ? "vec" : "general";
        if (p->narrow) snprintf(p->plan, sizeof p->plan, "depth=k_narrow<%s,%s>;frames=%d", p->dither ? ordered::name : none::name, path, frames);
        else snprintf(p->plan, sizeof p->plan, "depth=k_widen<%s>;frames=%d", path, frames);
    }

    static Args make_args(const H* p, bool fits, const Batch&) {
        Args a{};
        a.row = (uint32_t)p->w * 3u;
        a.lanes_row = (uint32_t)p->w / 8u;
        a.len = !fits ? 0u : p->narrow ? (uint32_t)p->h * a.lanes_row : (uint32_t)p->samples;
        return a;
    }

    static void launch(const H* p, bool fits, Args& a, int, unsigned g, hipStream_t st) {
        const unsigned lanes = p->narrow ? a.len : (a.len + 15u) / 16u;     // vec: of one frame
        const dim3 grid = fits ? dim3((lanes + BLOCK - 1) / BLOCK, 1, g) : dim3((a.row + BLOCK - 1) / BLOCK, p->h, g);
        if (!p->narrow) {
            if (fits) hipLaunchKernelGGL((k_widen<vec>), grid, dim3(BLOCK), 0, st, a);
            else hipLaunchKernelGGL((k_widen<general>), grid, dim3(BLOCK), 0, st, a);
        } else if (p->dither) {
            if (fits) hipLaunchKernelGGL((k_narrow<ordered, vec>), grid, dim3(BLOCK), 0, st, a);
            else hipLaunchKernelGGL((k_narrow<ordered, general>), grid, dim3(BLOCK), 0, st, a);
        } else {
            if (fits) hipLaunchKernelGGL((k_narrow<none, vec>), grid, dim3(BLOCK), 0, st, a);
            else hipLaunchKernelGGL((k_narrow<none, general>), grid, dim3(BLOCK), 0, st, a);
        }
    }
};

}  // namespace

extern "C" {

const char* crtfx_depth_last_error(const crtfx_depth* p) { return p ? p->err.c_str() : create_err<crtfx_depth>().c_str(); }

int crtfx_depth_create(int device, int h, int w, int direction, int dither, crtfx_depth** out_plan) {
    using H = crtfx_depth;
    if (const int rc = crtfx_frames::begin_create(out_plan)) return rc;
    if (const int rc = crtfx_frames::check_size<H>("h", h)) return rc;
    if (const int rc = crtfx_frames::check_size<H>("w", w)) return rc;
    if (direction != CRTFX_DEPTH_WIDEN && direction != CRTFX_DEPTH_NARROW) return fail<H>(nullptr, CRTFX_E_INVALID, "unknown direction %d", direction);
    if (dither != CRTFX_DITHER_NONE && dither != CRTFX_DITHER_ORDERED) return fail<H>(nullptr, CRTFX_E_INVALID, "unknown dither %d", dither);
    if (direction == CRTFX_DEPTH_WIDEN && dither != CRTFX_DITHER_NONE)
        return fail<H>(nullptr, CRTFX_E_INVALID, "dither = %d with direction = widen: widening is exact, there is nothing to dither", dither);
    return crtfx_frames::new_plan<U>(device, out_plan, [&](H* p) {
        p->h = h; p->w = w;
        p->narrow = direction == CRTFX_DEPTH_NARROW; p->dither = dither == CRTFX_DITHER_ORDERED;
        p->samples = (size_t)h * w * 3;
        p->src_bps = p->narrow ? 2 : 1; p->dst_bps = p->narrow ? 1 : 2;
        p->src_bytes = p->samples * p->src_bps;
        p->dst_bytes = p->samples * p->dst_bps;
        return CRTFX_OK;
    });
}

int crtfx_depth_destroy(crtfx_depth* p) { return crtfx_frames::destroy(p); }

int crtfx_depth_set_option(crtfx_depth* p, int option, int value) { return crtfx_frames::set_option<U>(p, option, value); }

int crtfx_depth_last_plan(crtfx_depth* p, char* buf, size_t n) { return crtfx_frames::last_plan(p, buf, n); }

int crtfx_depth_run(crtfx_depth* p, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream) {
    return crtfx_frames::run<U>(p, Batch{nullptr, src_base, src_stride_bytes, dst_base, dst_stride_bytes, n}, stream);
}

}  // extern "C"

