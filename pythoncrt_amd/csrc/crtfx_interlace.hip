// crtfx_interlace.hip — the interlace stage (include/crtfx_interlace.h): two consecutive h x w x 3 frames are woven into one interlaced
// frame, with an optional vertical low-pass inside each field's own frame.  A vec and a general kernel per (low-pass, sample type), the host
// glue, the C entry points.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <type_traits>

#include "crtfx_interlace.h"
#include "crtfx_edge.hip.h"
#include "crtfx_frame_host.h"

namespace crtfx_interlace_impl {

using namespace crtfx_deint_impl;       // the path tags, u8 / f16 with the quarter-code quantiser, load_dwords / store_dwords, BLOCK

// The low-pass settings: the rows a result reaches on either side of its own, and the rule on the codes r[k + reach] = r(k).  M is the
// largest code (255, or 1020 quarter codes).
struct none {
    static constexpr const char* name = "none";
    static constexpr int reach = 0;
};
struct linear {
    static constexpr const char* name = "linear";
    static constexpr int reach = 1;
    template <int M> static __device__ __forceinline__ int apply(const int (&r)[3]) { return (r[0] + 2 * r[1] + r[2] + 2) >> 2; }
    // the same on codes held as floats: every value is an integer below 2^24, so each step is exact and the floor is the shift
    template <int M> static __device__ __forceinline__ float apply(const float (&r)[3]) { return floorf((r[0] + 2.0f * r[1] + r[2] + 2.0f) * 0.25f); }
};
struct complex {
    static constexpr const char* name = "complex";
    static constexpr int reach = 2;
    template <int M> static __device__ __forceinline__ int apply(const int (&r)[5]) {
        int v = (-r[0] + 2 * r[1] + 6 * r[2] + 2 * r[3] - r[4] + 4) >> 3;      // -2040 .. 10204 before the shift, which is arithmetic: a floor
        v = v < 0 ? 0 : v;
        v = v > M ? M : v;
        return r[1] + r[3] > 2 * r[2] ? (v > r[2] ? v : r[2]) : (v < r[2] ? v : r[2]);
    }
    template <int M> static __device__ __forceinline__ float apply(const float (&r)[5]) {
        float v = floorf((2.0f * (r[1] + r[3]) + 6.0f * r[2] - (r[0] + r[4]) + 4.0f) * 0.125f);
        v = fminf(fmaxf(v, 0.0f), (float)M);
        return r[1] + r[3] > 2.0f * r[2] ? fmaxf(v, r[2]) : fminf(v, r[2]);
    }
};

// The quarter codes of a dword's two halves as floats: f16::codes (crtfx_edge.hip.h) without the conversion to integers.
__device__ __forceinline__ void half_codes(uint32_t dword, float (&q)[2]) {
    typedef _Float16 half2 __attribute__((ext_vector_type(2)));
    half2 t = __builtin_bit_cast(half2, dword) * (half2)(_Float16)4.0f;
    t = __builtin_elementwise_max(t, (half2)(_Float16)0.0f);
    t = __builtin_elementwise_min(t, (half2)(_Float16)1020.0f);
    t = __builtin_elementwise_rint(t);
    q[0] = (float)t.x; q[1] = (float)t.y;
}

// Launch constants.
struct Args {
    const uint8_t* src;
    uint8_t* dst;
    size_t src_stride, dst_stride;      // bytes; the destination's is per OUTPUT frame
    uint32_t h, w;
    uint32_t blocks_row;                // vec: 8-pixel blocks per row (w / 8)
    uint32_t lanes;                     // vec: lanes per output frame (h * blocks_row)
    uint32_t first;                     // the parity of the rows frame A gives: 0 under TFF, 1 under BFF
    uint32_t n;                         // source frames of this launch: output frame z is woven from 2 z and min(2 z + 1, n - 1)
};

// the frame of this launch's source that gives row y of output frame z
__device__ __forceinline__ const uint8_t* field_frame(const Args& a, uint32_t z, uint32_t y) {
    const uint32_t fa = 2u * z, fb = fa + 1u < a.n ? fa + 1u : a.n - 1u;
    return a.src + (size_t)((y & 1u) == a.first ? fa : fb) * a.src_stride;
}

// row clamp(y + k, 0, h - 1)
__device__ __forceinline__ uint32_t clamp_row(uint32_t y, int k, uint32_t h) {
    const int yy = (int)y + k;
    return yy < 0 ? 0u : ((uint32_t)yy < h ? (uint32_t)yy : h - 1u);
}

// the byte offset of that row from row y, |k| <= 2: at most two rows of at most 32767 * 6 bytes to either side, a 24-bit product (one
// 64-bit product per row costs more than LINEAR's filter)
__device__ __forceinline__ ptrdiff_t clamp_row_delta(size_t row, uint32_t y, int k, uint32_t h) {
    return (ptrdiff_t)__mul24((int)clamp_row(y, k, h) - (int)y, (int)row);
}

// vec: one lane per 1 row x 8 pixels of an OUTPUT frame
template <class L, class P>
__device__ __forceinline__ void interlace_vec(const Args& a) {
    constexpr int SZ = sizeof(typename P::T), SPD = P::SPD, CD = 24 / SPD, R = L::reach;
    constexpr int M = SZ == 1 ? 255 : 1020;
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.lanes) return;
    const uint32_t y = i / a.blocks_row, bx = i - y * a.blocks_row;
    const size_t row = (size_t)a.w * 3u * SZ, col = (size_t)bx * 24u * SZ;
    const uint8_t* __restrict__ s = field_frame(a, blockIdx.z, y) + col;
    uint8_t* __restrict__ d = a.dst + (size_t)blockIdx.z * a.dst_stride + (size_t)y * row + col;
    uint32_t out[CD];
    if constexpr (R == 0) {                                             // the row's bits
        load_dwords<CD>(s + (size_t)y * row, out);
    } else {
        uint32_t wd[2 * R + 1][CD];
#pragma unroll
        for (int k = -R; k <= R; ++k) load_dwords<CD>(s + (size_t)y * row + clamp_row_delta(row, y, k, a.h), wd[k + R]);
#pragma unroll
        for (int j = 0; j < CD; ++j) {
            if constexpr (SZ == 1 && R == 1) {                          // (a + 2 b + c + 2) >> 2 of four bytes as two pairs of 16-bit sums (at most 1022)
                const uint32_t lo = (wd[0][j] & 0x00ff00ffu) + 2u * (wd[1][j] & 0x00ff00ffu) + (wd[2][j] & 0x00ff00ffu) + 0x00020002u;
                const uint32_t hi = ((wd[0][j] >> 8) & 0x00ff00ffu) + 2u * ((wd[1][j] >> 8) & 0x00ff00ffu) + ((wd[2][j] >> 8) & 0x00ff00ffu) + 0x00020002u;
                out[j] = ((lo >> 2) & 0x00ff00ffu) | (((hi >> 2) & 0x00ff00ffu) << 8);
            } else if constexpr (SZ == 2) {                             // halves: the codes stay floats from the quantiser to half(r / 4), which is exact
                float q[2 * R + 1][2], v[2];
#pragma unroll
                for (int k = 0; k <= 2 * R; ++k) half_codes(wd[k][j], q[k]);
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    float r[2 * R + 1];
#pragma unroll
                    for (int k = 0; k <= 2 * R; ++k) r[k] = q[k][t];
                    v[t] = L::template apply<M>(r) * 0.25f;
                }
                out[j] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(v[0], v[1]));
            } else {
                int q[2 * R + 1][SPD];
#pragma unroll
                for (int k = 0; k <= 2 * R; ++k) P::codes(wd[k][j], q[k]);
                uint32_t o = 0u;
#pragma unroll
                for (int t = 0; t < SPD; ++t) {
                    int r[2 * R + 1];
#pragma unroll
                    for (int k = 0; k <= 2 * R; ++k) r[k] = q[k][t];
                    o |= P::bits(L::template apply<M>(r)) << (8 * SZ * t);
                }
                out[j] = o;
            }
        }
    }
    store_dwords<CD>(d, out);
}

// general: one lane per pixel of an OUTPUT frame
template <class L, class P>
__device__ __forceinline__ void interlace_general(const Args& a) {
    typedef typename P::T T;
    constexpr int R = L::reach, M = sizeof(T) == 1 ? 255 : 1020;
    const uint32_t x = blockIdx.x * BLOCK + threadIdx.x, y = blockIdx.y;
    if (x >= a.w) return;
    const size_t row = (size_t)a.w * 3u, o = (size_t)x * 3u;
    const T* __restrict__ s = reinterpret_cast<const T*>(field_frame(a, blockIdx.z, y)) + o;
    T* __restrict__ d = reinterpret_cast<T*>(a.dst + (size_t)blockIdx.z * a.dst_stride) + (size_t)y * row + o;
    if constexpr (R == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] = s[(size_t)y * row + c];
    } else {
        const T* __restrict__ rows[2 * R + 1];
#pragma unroll
        for (int k = -R; k <= R; ++k) rows[k + R] = s + (ptrdiff_t)y * (ptrdiff_t)row + clamp_row_delta(row, y, k, a.h);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            int r[2 * R + 1];
#pragma unroll
            for (int k = 0; k <= 2 * R; ++k) r[k] = P::code(rows[k][c]);
            d[c] = (T)P::bits(L::template apply<M>(r));
        }
    }
}

template <class L, class P, class Path>
__global__ __launch_bounds__(BLOCK) void k_interlace(Args a) {
    if constexpr (std::is_same<Path, vec>::value) interlace_vec<L, P>(a); else interlace_general<L, P>(a);
}

}  // namespace crtfx_interlace_impl

using namespace crtfx_interlace_impl;

struct crtfx_interlace : crtfx_frames::Plan {  // one frame size and sample type on both sides; frames_in = 2
    int h = 0, w = 0, lowpass = 0;
    bool half = false, bff = false;
};

namespace {

using crtfx_frames::Batch;
using crtfx_stage::create_err;
using crtfx_stage::fail;

template <class L, class P>
void launch_path(bool fits, dim3 grid, hipStream_t st, const Args& a) {
    if (fits) hipLaunchKernelGGL((k_interlace<L, P, vec>), grid, dim3(BLOCK), 0, st, a);
    else hipLaunchKernelGGL((k_interlace<L, P, general>), grid, dim3(BLOCK), 0, st, a);
}

template <class L>
void launch_pix(const crtfx_interlace* p, bool fits, dim3 grid, hipStream_t st, const Args& a) {
    if (p->half) launch_path<L, f16>(fits, grid, st, a); else launch_path<L, u8>(fits, grid, st, a);
}

const char* lowpass_name(int lowpass) {
    return lowpass == CRTFX_INTERLACE_COMPLEX ? complex::name : lowpass == CRTFX_INTERLACE_LINEAR ? linear::name : none::name;
}

struct U : crtfx_frames::Unit {
    using H = crtfx_interlace;
    static constexpr int force_option = CRTFX_INTERLACE_OPT_FORCE_GENERAL;
    static constexpr const char* name = "interlace";
    static constexpr bool one_size = true;

    // the vec kernels' conditions (crtfx_interlace.h); b.n counts source frames, of which ceil(n / 2) frames are written
    static bool vec_fits(const H* p, const Batch& b) {
        if (p->force_general || (p->w & 7)) return false;
        if ((reinterpret_cast<uintptr_t>(b.src) | reinterpret_cast<uintptr_t>(b.dst)) & 3u) return false;
        if (b.n > 1 && (b.src_stride & 3u)) return false;
        return b.n <= 2 || !(b.dst_stride & 3u);
    }

    static void note_plan(H* p, bool fits, int frames) {
        snprintf(p->plan, sizeof p->plan, "interlace=k_interlace<%s,%s,%s>;frames=%d", lowpass_name(p->lowpass), p->half ? f16::name : u8::name,
                 fits ? vec::name : general::name, frames);
    }

    static Args make_args(const H* p, bool, const Batch&) {
        Args a{};
        a.h = (uint32_t)p->h; a.w = (uint32_t)p->w;
        a.blocks_row = a.w / 8u;
        a.lanes = a.h * a.blocks_row;                                   // below 2^27
        a.first = p->bff ? 1u : 0u;
        return a;
    }

    // g source frames from an even frame of the batch on (Unit::group is even): (g + 1) / 2 output frames, the last one of an odd g woven with itself
    static void launch(const H* p, bool fits, Args& a, int, unsigned g, hipStream_t st) {
        a.n = g;
        const unsigned z = (g + 1u) / 2u;
        const dim3 grid = fits ? dim3((a.lanes + BLOCK - 1) / BLOCK, 1, z) : dim3((a.w + BLOCK - 1) / BLOCK, p->h, z);
        if (p->lowpass == CRTFX_INTERLACE_COMPLEX) launch_pix<complex>(p, fits, grid, st, a);
        else if (p->lowpass == CRTFX_INTERLACE_LINEAR) launch_pix<linear>(p, fits, grid, st, a);
        else launch_pix<none>(p, fits, grid, st, a);
    }
};

}  // namespace

extern "C" {

const char* crtfx_interlace_last_error(const crtfx_interlace* p) { return p ? p->err.c_str() : create_err<crtfx_interlace>().c_str(); }

int crtfx_interlace_create(int device, int h, int w, int pix_fmt, int order, int lowpass, crtfx_interlace** out_plan) {
    using H = crtfx_interlace;
    if (const int rc = crtfx_frames::begin_create(out_plan)) return rc;
    if (h < 2 || h > 32767) return fail<H>(nullptr, CRTFX_E_INVALID, "h = %d outside 2..32767 (a frame of two fields has two rows)", h);
    if (const int rc = crtfx_frames::check_size<H>("w", w)) return rc;
    if (pix_fmt != CRTFX_PIX_U8 && pix_fmt != CRTFX_PIX_F16) return fail<H>(nullptr, CRTFX_E_INVALID, "unknown pix_fmt %d", pix_fmt);
    if (order != CRTFX_INTERLACE_TFF && order != CRTFX_INTERLACE_BFF) return fail<H>(nullptr, CRTFX_E_INVALID, "unknown order %d", order);
    if (lowpass != CRTFX_INTERLACE_NONE && lowpass != CRTFX_INTERLACE_LINEAR && lowpass != CRTFX_INTERLACE_COMPLEX)
        return fail<H>(nullptr, CRTFX_E_INVALID, "unknown lowpass %d", lowpass);
    return crtfx_frames::new_plan<U>(device, out_plan, [&](H* p) {
        p->h = h; p->w = w; p->lowpass = lowpass;
        p->half = pix_fmt == CRTFX_PIX_F16; p->bff = order == CRTFX_INTERLACE_BFF;
        p->src_bps = p->dst_bps = p->half ? 2 : 1;
        p->src_bytes = p->dst_bytes = (size_t)h * w * 3 * p->src_bps;
        p->frames_in = 2;
        return CRTFX_OK;
    });
}

int crtfx_interlace_frames_in(const crtfx_interlace* p) { return p ? p->frames_in : 0; }

int crtfx_interlace_destroy(crtfx_interlace* p) { return crtfx_frames::destroy(p); }

int crtfx_interlace_set_option(crtfx_interlace* p, int option, int value) { return crtfx_frames::set_option<U>(p, option, value); }

int crtfx_interlace_last_plan(crtfx_interlace* p, char* buf, size_t n) { return crtfx_frames::last_plan(p, buf, n); }

int crtfx_interlace_run(crtfx_interlace* p, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream) {
    return crtfx_frames::run<U>(p, Batch{nullptr, src_base, src_stride_bytes, dst_base, dst_stride_bytes, n}, stream);
}

}  // extern "C"
