// crtfx_444.hip — the 10-bit 4:4:4 pair of libcrtfx.so (include/crtfx_444.h): yuv444p10le / gbrp10le / x2rgb10le frames -> half RGB in front
// of a half chain (crtfx_unpack444_*), finished half RGB frames -> the same layouts behind it (crtfx_egress444_*).  A translation unit of its
// own: it shares no kernel, table or handle with the effect chain, the ingest stage or the other source and egress stages.  The host code around the kernels (checks, frame-group loop, error strings) is
// the skeleton of crtfx_stage_host.h: host templates only, so nothing is shared at run time either.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "crtfx_444.h"
#include "crtfx_stage_host.h"

namespace crtfx_444_impl {

constexpr int BLOCK = 256;
constexpr int SH = 16;                          // fractional bits of the matrix
constexpr int GENERAL = 0, VEC = 1;             // the PATH template argument; LAYOUT is a crtfx_444_layout
constexpr unsigned QMAX = 1020u;                // the largest quarter code: 255.0 on the half scale
constexpr unsigned CMAX = 1023u;                // the largest 10-bit code

struct Args {
    const uint8_t* src; size_t src_stride;
    uint8_t* dst; size_t dst_stride;
    int h, w;
    int m[9];                                   // source: rows R, G, B over P0, P1, P2; egress: rows T0, T1, T2 over R, G, B
    int k[3];                                   // source: off; egress: (off << SH) + half
};

// unsigned dwords at 4-byte alignment: the widest access the vec path's rule (crtfx_444.h) guarantees
struct __attribute__((packed, aligned(4))) U4 { unsigned v[4]; };
struct __attribute__((packed, aligned(4))) U12 { unsigned v[12]; };

// 16-bit word i (0..7) of eight words held as four dwords
__device__ __forceinline__ unsigned word16(const U4& d, int i) { return (i & 1) ? d.v[i >> 1] >> 16 : d.v[i >> 1] & 0xFFFFu; }

// ---- source: 10-bit 4:4:4 -> half RGB ----

// clamp(acc >> SH, 0, 1020) of a signed accumulator in the form of the other source kernels (crtfx_unpack.hip says why): lower clamp on the
// accumulator, a LOGICAL shift of the non-negative rest, an unsigned minimum.
__device__ __forceinline__ unsigned quarter(int acc) { return min((unsigned)max(acc, 0) >> SH, QMAX); }

// the half bit pattern of quarter code q, q / 4 on the 0..255 scale: exact, every quarter code is a half (no rounding occurs)
__device__ __forceinline__ unsigned half_bits(unsigned q) { return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)((float)q * 0.25f)); }

// the three half patterns of one pixel from its three 10-bit samples
__device__ __forceinline__ void pixel(const Args& a, unsigned p0, unsigned p1, unsigned p2, unsigned out[3]) {
    const int c0 = (int)p0 - a.k[0], c1 = (int)p1 - a.k[1], c2 = (int)p2 - a.k[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = half_bits(quarter(a.m[3 * k] * c0 + a.m[3 * k + 1] * c1 + a.m[3 * k + 2] * c2 + (1 << (SH - 1))));
}

// vec (w % 8 == 0, 4-byte-aligned frame bases): one lane = one row of 8 columns of one frame, 3 x 16 (planar) or 2 x 16 (x2rgb10le) bytes
// in, 48 bytes out; consecutive lanes, consecutive column blocks.
// general: one lane = one pixel; 16-bit accesses (32-bit ones on the x2rgb10le side), any size.
template <int LAYOUT, int PATH>
__global__ __launch_bounds__(BLOCK) void k_unpack10_444(Args a) {
    const uint8_t* fsrc = a.src + (size_t)blockIdx.z * a.src_stride;
    uint8_t* fdst = a.dst + (size_t)blockIdx.z * a.dst_stride;
    const int idx = blockIdx.x * BLOCK + threadIdx.x;
    const size_t plane = (size_t)a.h * a.w * 2;             // bytes of one plane
    if (PATH == VEC) {
        const int nbx = a.w >> 3;
        if (idx >= a.h * nbx) return;
        const int y = idx / nbx, bx = idx - y * nbx;
        const size_t px = (size_t)y * a.w + (size_t)bx * 8;  // the lane's first pixel
        unsigned hb[24];                                    // 8 pixels x (R, G, B)
        if (LAYOUT == CRTFX_444_PLANAR) {
            const U4 s0 = *reinterpret_cast<const U4*>(fsrc + px * 2);
            const U4 s1 = *reinterpret_cast<const U4*>(fsrc + plane + px * 2);
            const U4 s2 = *reinterpret_cast<const U4*>(fsrc + 2 * plane + px * 2);
#pragma unroll
            for (int p = 0; p < 8; ++p) pixel(a, word16(s0, p) & CMAX, word16(s1, p) & CMAX, word16(s2, p) & CMAX, hb + 3 * p);
        } else {
            const U4 lo = *reinterpret_cast<const U4*>(fsrc + px * 4);
            const U4 hi = *reinterpret_cast<const U4*>(fsrc + px * 4 + 16);
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const unsigned d = p < 4 ? lo.v[p] : hi.v[p - 4];
                pixel(a, (d >> 20) & CMAX, (d >> 10) & CMAX, d & CMAX, hb + 3 * p);
            }
        }
        U12 o;
#pragma unroll
        for (int i = 0; i < 12; ++i) o.v[i] = hb[2 * i] | (hb[2 * i + 1] << 16);
        *reinterpret_cast<U12*>(fdst + px * 6) = o;
    } else {
        if (idx >= a.h * a.w) return;                       // idx = y * w + x
        unsigned p0, p1, p2;
        if (LAYOUT == CRTFX_444_PLANAR) {
            const uint16_t* s = reinterpret_cast<const uint16_t*>(fsrc) + idx;
            const size_t pw = (size_t)a.h * a.w;
            p0 = s[0] & CMAX; p1 = s[pw] & CMAX; p2 = s[2 * pw] & CMAX;
        } else {
            const unsigned d = reinterpret_cast<const unsigned*>(fsrc)[idx];
            p0 = (d >> 20) & CMAX; p1 = (d >> 10) & CMAX; p2 = d & CMAX;
        }
        unsigned hb[3];
        pixel(a, p0, p1, p2, hb);
        uint16_t* out = reinterpret_cast<uint16_t*>(fdst) + (size_t)idx * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = (uint16_t)hb[k];
    }
}

// ---- egress: half RGB -> 10-bit 4:4:4 ----

// the quarter code of a half bit pattern: rint_to_even(min(max(4 f, 0), 1020)), NaN -> 0 — crtfx_deep.h's quantiser.  The half -> float
// conversion and 4 f are exact; the comparisons are written out so that a NaN (either kind) fails `> 0` and takes the 0, as -0, negatives
// and -inf do; +inf takes 1020.
__device__ __forceinline__ int quantise(unsigned bits16) {
    float t = 4.0f * (float)__builtin_bit_cast(_Float16, (unsigned short)bits16);
    t = t > 0.0f ? t : 0.0f;
    t = t < 1020.0f ? t : 1020.0f;
    return (int)rintf(t);
}

// crtfx_egress444_create admits only matrices whose accumulators stay in [0, 2^31): the lower clamp can never act, the shift is a logical one
// and the upper clamp is an unsigned minimum (the form of crtfx_egress.hip, for the reason given there).
__device__ __forceinline__ unsigned sample10(const Args& a, int row, const int q[3]) {
    return min((unsigned)(a.m[3 * row] * q[0] + a.m[3 * row + 1] * q[1] + a.m[3 * row + 2] * q[2] + a.k[row]) >> SH, CMAX);
}

// vec: one lane = one row of 8 columns, 48 bytes in, 3 x 16 or 2 x 16 bytes out; general: one lane = one pixel.
template <int LAYOUT, int PATH>
__global__ __launch_bounds__(BLOCK) void k_egress10_444(Args a) {
    const uint8_t* fsrc = a.src + (size_t)blockIdx.z * a.src_stride;
    uint8_t* fdst = a.dst + (size_t)blockIdx.z * a.dst_stride;
    const int idx = blockIdx.x * BLOCK + threadIdx.x;
    const size_t plane = (size_t)a.h * a.w * 2;             // bytes of one plane
    if (PATH == VEC) {
        const int nbx = a.w >> 3;
        if (idx >= a.h * nbx) return;
        const int y = idx / nbx, bx = idx - y * nbx;
        const size_t px = (size_t)y * a.w + (size_t)bx * 8;
        const U12 rgb = *reinterpret_cast<const U12*>(fsrc + px * 6);
        unsigned t[8][3];
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            int q[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int i = 3 * p + c;
                q[c] = quantise((i & 1) ? rgb.v[i >> 1] >> 16 : rgb.v[i >> 1] & 0xFFFFu);
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) t[p][j] = sample10(a, j, q);
        }
        if (LAYOUT == CRTFX_444_PLANAR) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                U4 o;
#pragma unroll
                for (int i = 0; i < 4; ++i) o.v[i] = t[2 * i][j] | (t[2 * i + 1][j] << 16);
                *reinterpret_cast<U4*>(fdst + (size_t)j * plane + px * 2) = o;
            }
        } else {
            U4 lo, hi;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                lo.v[p] = (t[p][0] << 20) | (t[p][1] << 10) | t[p][2];
                hi.v[p] = (t[p + 4][0] << 20) | (t[p + 4][1] << 10) | t[p + 4][2];
            }
            *reinterpret_cast<U4*>(fdst + px * 4) = lo;
            *reinterpret_cast<U4*>(fdst + px * 4 + 16) = hi;
        }
    } else {
        if (idx >= a.h * a.w) return;                       // idx = y * w + x
        const uint16_t* s = reinterpret_cast<const uint16_t*>(fsrc) + (size_t)idx * 3;
        int q[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c] = quantise(s[c]);
        const unsigned t0 = sample10(a, 0, q), t1 = sample10(a, 1, q), t2 = sample10(a, 2, q);
        if (LAYOUT == CRTFX_444_PLANAR) {
            uint16_t* out = reinterpret_cast<uint16_t*>(fdst) + idx;
            const size_t pw = (size_t)a.h * a.w;
            out[0] = (uint16_t)t0; out[pw] = (uint16_t)t1; out[2 * pw] = (uint16_t)t2;
        } else {
            reinterpret_cast<unsigned*>(fdst)[idx] = (t0 << 20) | (t1 << 10) | t2;
        }
    }
}

struct Plan : crtfx_stage::StagePlan { Args args{}; };         // what the two handle families share, told apart by `egress`

}  // namespace crtfx_444_impl

using namespace crtfx_444_impl;
using namespace crtfx_stage;

struct crtfx_unpack444 : Plan {};
struct crtfx_egress444 : Plan {};

namespace {

static_assert(SH == MATRIX_SH, "the row checks of crtfx_stage_host.h assume this matrix scale");
static_assert((int)CRTFX_UNPACK444_OPT_FORCE_GENERAL == (int)CRTFX_EGRESS444_OPT_FORCE_GENERAL, "one option number for both families");

template <int LAYOUT>
void launch_layout(const Plan* p, bool vec, dim3 grid, hipStream_t st, const Args& a) {
    if (p->egress) {
        if (vec) hipLaunchKernelGGL((k_egress10_444<LAYOUT, VEC>), grid, dim3(BLOCK), 0, st, a);
        else hipLaunchKernelGGL((k_egress10_444<LAYOUT, GENERAL>), grid, dim3(BLOCK), 0, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((k_unpack10_444<LAYOUT, VEC>), grid, dim3(BLOCK), 0, st, a);
        else hipLaunchKernelGGL((k_unpack10_444<LAYOUT, GENERAL>), grid, dim3(BLOCK), 0, st, a);
    }
}

struct Unit {
    static constexpr int block = BLOCK, force_option = CRTFX_UNPACK444_OPT_FORCE_GENERAL;
    static const char* name(bool egress) { return egress ? "egress444" : "unpack444"; }
    static void note_plan(Plan* p, bool vec, int frames) {
        const char* kernel = p->egress ? "egress444=k_egress10_444" : "unpack444=k_unpack10_444";
        snprintf(p->plan, sizeof p->plan, "%s<%s,%s>;frames=%d", kernel, p->layout == CRTFX_444_X2RGB10LE ? "x2rgb10le" : "planar", vec ? "vec" : "general", frames);
    }
    // the half side holds 16-bit words; the 10-bit side 16-bit (planar) or 32-bit (x2rgb10le) ones
    static int check_alignment(Plan* p, const void* src_base, size_t src_stride_bytes, const void* dst_base, size_t dst_stride_bytes) {
        const uintptr_t rgb_side = p->egress ? reinterpret_cast<uintptr_t>(src_base) | src_stride_bytes : reinterpret_cast<uintptr_t>(dst_base) | dst_stride_bytes;
        const uintptr_t deep_side = p->egress ? reinterpret_cast<uintptr_t>(dst_base) | dst_stride_bytes : reinterpret_cast<uintptr_t>(src_base) | src_stride_bytes;
        if (rgb_side & 1u) return fail(p, CRTFX_E_INVALID, "an odd half-frame base or stride: 16-bit samples need 2-byte alignment");
        if (p->layout == CRTFX_444_X2RGB10LE) {
            if (deep_side & 3u) return fail(p, CRTFX_E_INVALID, "an x2rgb10le frame base or stride is no multiple of 4: 32-bit words need 4-byte alignment");
        } else if (deep_side & 1u) {
            return fail(p, CRTFX_E_INVALID, "an odd planar frame base or stride: 16-bit samples need 2-byte alignment");
        }
        return CRTFX_OK;
    }
    static int items(const Args& a, bool vec) { return vec ? a.h * (a.w >> 3) : a.h * a.w; }           // at most 32767 * 32767 < 2^30
    static void launch(const Plan* p, bool vec, dim3 grid, hipStream_t st, const Args& a) {
        if (p->layout == CRTFX_444_X2RGB10LE) launch_layout<CRTFX_444_X2RGB10LE>(p, vec, grid, st, a);
        else launch_layout<CRTFX_444_PLANAR>(p, vec, grid, st, a);
    }
};

template <class H>
int create(bool egress, int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, H** out_plan) {
    if (const int rc = begin_create(out_plan)) return rc;
    if (pix_fmt == CRTFX_PIX_U8)
        return fail<H>(nullptr, CRTFX_E_UNSUPPORTED, "only half RGB frames are %s (the 10-bit 4:4:4 stages have no uint8 path)", egress ? "converted" : "written");
    if (const int rc = check_create<H>(pix_fmt, CRTFX_PIX_F16, h, w, layout, layout == CRTFX_444_PLANAR || layout == CRTFX_444_X2RGB10LE, m, off, CMAX)) return rc;
    long long k[3] = {off[0], off[1], off[2]};
    if (egress) {
        for (int i = 0; i < 3; ++i) {
            k[i] = ((long long)off[i] << SH) + (1LL << (SH - 1));
            if (!egress_row_fits(m + 3 * i, k[i], QMAX)) return fail<H>(nullptr, CRTFX_E_INVALID, "the matrix lets an accumulator leave [0, 2^31)");
        }
    } else if (!source_row_fits(m, CMAX) || !source_row_fits(m + 3, CMAX) || !source_row_fits(m + 6, CMAX)) {
        return fail<H>(nullptr, CRTFX_E_INVALID, "the matrix lets an accumulator leave int32");
    }
    H* p = nullptr;
    if (const int rc = new_plan(egress, device, layout, h, w, m, &p)) return rc;
    for (int i = 0; i < 3; ++i) p->args.k[i] = (int)k[i];
    p->frame_bytes = (size_t)h * w * (layout == CRTFX_444_X2RGB10LE ? 4 : 6);
    p->rgb_bytes = (size_t)h * w * 6;
    Unit::note_plan(p, vec_fits(p, nullptr, 0, nullptr, 0, 1), 0);
    *out_plan = p;
    return CRTFX_OK;
}

}  // namespace

extern "C" {

const char* crtfx_unpack444_last_error(const crtfx_unpack444* p) { return p ? p->err.c_str() : create_err<crtfx_unpack444>().c_str(); }
int crtfx_unpack444_create(int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, crtfx_unpack444** out_plan) {
    return create(false, device, h, w, pix_fmt, layout, m, off, out_plan);
}
int crtfx_unpack444_destroy(crtfx_unpack444* p) { return destroy(p); }
size_t crtfx_unpack444_frame_bytes(const crtfx_unpack444* p) { return p ? p->frame_bytes : 0; }
int crtfx_unpack444_set_option(crtfx_unpack444* p, int option, int value) { return set_option<Unit>(p, option, value); }
int crtfx_unpack444_last_plan(crtfx_unpack444* p, char* buf, size_t n) { return last_plan(p, buf, n); }
int crtfx_unpack444_run(crtfx_unpack444* p, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream) {
    return run_frames<Unit>(p, src_base, src_stride_bytes, dst_base, dst_stride_bytes, n, stream);
}

const char* crtfx_egress444_last_error(const crtfx_egress444* p) { return p ? p->err.c_str() : create_err<crtfx_egress444>().c_str(); }
int crtfx_egress444_create(int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, crtfx_egress444** out_plan) {
    return create(true, device, h, w, pix_fmt, layout, m, off, out_plan);
}
int crtfx_egress444_destroy(crtfx_egress444* p) { return destroy(p); }
size_t crtfx_egress444_frame_bytes(const crtfx_egress444* p) { return p ? p->frame_bytes : 0; }
int crtfx_egress444_set_option(crtfx_egress444* p, int option, int value) { return set_option<Unit>(p, option, value); }
int crtfx_egress444_last_plan(crtfx_egress444* p, char* buf, size_t n) { return last_plan(p, buf, n); }
int crtfx_egress444_run(crtfx_egress444* p, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream) {
    return run_frames<Unit>(p, src_base, src_stride_bytes, dst_base, dst_stride_bytes, n, stream);
}

}  // extern "C"
