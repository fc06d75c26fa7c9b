// crtfx_422.hip — the 8-bit 4:2:2 pair of libcrtfx.so (include/crtfx_422.h): uint8 yuv422p / yuyv422 / uyvy422 frames -> uint8 RGB in front
// of the chain (crtfx_unpack422_*), finished uint8 RGB frames -> the same three layouts behind it (crtfx_egress422_*).
// A translation unit of its own: it shares no kernel, table or handle with the effect chain, the ingest stage or the 4:2:0 stages.  The host code around the kernels (checks, frame-group loop, error strings) is
// the skeleton of crtfx_stage_host.h: host templates only, so nothing is shared at run time either.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "crtfx_422.h"
#include "crtfx_stage_host.h"

namespace crtfx_422_impl {

constexpr int BLOCK = 256;
constexpr int SH = 16;                          // fractional bits of the matrix; a chroma sum of two samples carries one more
constexpr int GENERAL = 0, VEC = 1;             // the PATH template argument; LAYOUT is a crtfx_422_layout

struct Args {
    const uint8_t* src; size_t src_stride;
    uint8_t* dst; size_t dst_stride;
    int h, w, cw;
    int m[9];                                   // source: rows R, G, B over Y, U, V; egress: rows Y, U, V over R, G, B
    int k[3];                                   // source: off; egress: (off0 << SH) + half, (off1,2 << (SH + 1)) + half
};

// unsigned dwords at 4-byte alignment: the widest access the vec path's rule (crtfx_422.h) guarantees
struct __attribute__((packed, aligned(4))) U2 { unsigned x, y; };
struct __attribute__((packed, aligned(4))) U4 { unsigned v[4]; };
struct __attribute__((packed, aligned(4))) U6 { unsigned v[6]; };

// byte positions inside a packed macropixel: yuyv422 = Y0 U Y1 V, uyvy422 = U Y0 V Y1
template <int LAYOUT> struct Mac {
    static constexpr int Y0 = LAYOUT == CRTFX_422_YUYV422 ? 0 : 1, Y1 = Y0 + 2, U = LAYOUT == CRTFX_422_YUYV422 ? 1 : 0, V = U + 2;
};

// ---- source ----

// clamp(acc >> SH, 0, 255) of a signed accumulator: lower clamp on the accumulator, a LOGICAL shift of the non-negative rest, an unsigned
// minimum.  The form of crtfx_unpack.hip, for the reason given there (the signed form of two neighbouring samples packed into one word is
// contracted to v_ashr_pk_u8_i32, whose upper destination bits the MI355X keeps while the compiler assumes them cleared).
__device__ __forceinline__ unsigned clamp8(int acc) { return min((unsigned)max(acc, 0) >> SH, 255u); }

// the chroma term of one chroma sample per output channel, rounding constant included: m[k][1] * d + m[k][2] * e + half
__device__ __forceinline__ void chroma_terms(const Args& a, int u, int v, int t[3]) {
    const int d = u - a.k[1], e = v - a.k[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = a.m[3 * k + 1] * d + a.m[3 * k + 2] * e + (1 << (SH - 1));
}

// vec (w % 8 == 0, 4-byte-aligned frame bases): one lane = one row of 8 columns of one frame; consecutive lanes, consecutive column blocks.
// general: one lane = one chroma sample and the (up to) two pixels under it; byte accesses only, any size and alignment.
template <int LAYOUT, int PATH>
__global__ __launch_bounds__(BLOCK) void k_unpack_422(Args a) {
    const uint8_t* fsrc = a.src + (size_t)blockIdx.z * a.src_stride;
    uint8_t* fdst = a.dst + (size_t)blockIdx.z * a.dst_stride;
    const int idx = blockIdx.x * BLOCK + threadIdx.x;
    if (PATH == VEC) {
        const int nbx = a.w >> 3;
        if (idx >= a.h * nbx) return;
        const int y = idx / nbx, bx = idx - y * nbx;
        unsigned yw[2], up, vp;                 // y0 .. y3 | y4 .. y7, u0 u1 u2 u3, v0 v1 v2 v3
        if (LAYOUT == CRTFX_422_YUV422P) {
            const U2 yy = *reinterpret_cast<const U2*>(fsrc + (size_t)y * a.w + (size_t)bx * 8);
            yw[0] = yy.x; yw[1] = yy.y;
            const uint8_t* cbase = fsrc + (size_t)a.h * a.w;
            const size_t o = (size_t)y * a.cw + (size_t)bx * 4;
            up = *reinterpret_cast<const unsigned*>(cbase + o);
            vp = *reinterpret_cast<const unsigned*>(cbase + (size_t)a.h * a.cw + o);
        } else {
            using M = Mac<LAYOUT>;
            const U4 mp = *reinterpret_cast<const U4*>(fsrc + (size_t)y * a.w * 2 + (size_t)bx * 16);      // four macropixels
            yw[0] = yw[1] = up = vp = 0u;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                yw[q >> 1] |= ((mp.v[q] >> (8 * M::Y0)) & 255u) << (16 * (q & 1));
                yw[q >> 1] |= ((mp.v[q] >> (8 * M::Y1)) & 255u) << (16 * (q & 1) + 8);
                up |= ((mp.v[q] >> (8 * M::U)) & 255u) << (8 * q);
                vp |= ((mp.v[q] >> (8 * M::V)) & 255u) << (8 * q);
            }
        }
        U6 o;
#pragma unroll
        for (int i = 0; i < 6; ++i) o.v[i] = 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {           // chroma sample q = columns 2q, 2q + 1
            int t[3];
            chroma_terms(a, (int)((up >> (8 * q)) & 255u), (int)((vp >> (8 * q)) & 255u), t);
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int p = 2 * q + e;
                const int c = (int)((yw[p >> 2] >> (8 * (p & 3))) & 255u) - a.k[0];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int b = 3 * p + k;
                    o.v[b >> 2] |= clamp8(a.m[3 * k] * c + t[k]) << (8 * (b & 3));
                }
            }
        }
        *reinterpret_cast<U6*>(fdst + (size_t)y * a.w * 3 + (size_t)bx * 24) = o;
    } else {
        if (idx >= a.h * a.cw) return;
        const int y = idx / a.cw, cx = idx - y * a.cw;
        const int x0 = 2 * cx;
        const bool right = x0 + 1 < a.w;
        int y0, y1 = 0, u, v;
        if (LAYOUT == CRTFX_422_YUV422P) {
            const uint8_t* yp = fsrc + (size_t)y * a.w + x0;
            y0 = yp[0];
            if (right) y1 = yp[1];
            const uint8_t* cbase = fsrc + (size_t)a.h * a.w;
            const size_t o = (size_t)y * a.cw + cx;
            u = cbase[o]; v = cbase[(size_t)a.h * a.cw + o];
        } else {
            using M = Mac<LAYOUT>;
            const uint8_t* mp = fsrc + ((size_t)y * a.cw + cx) * 4;
            y0 = mp[M::Y0]; u = mp[M::U]; v = mp[M::V];
            if (right) y1 = mp[M::Y1];          // the pad byte of an odd row is not looked at
        }
        int t[3];
        chroma_terms(a, u, v, t);
        uint8_t* out = fdst + ((size_t)y * a.w + x0) * 3;
        const int c0 = y0 - a.k[0], c1 = y1 - a.k[0];
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = (uint8_t)clamp8(a.m[3 * k] * c0 + t[k]);
        if (right) {
#pragma unroll
            for (int k = 0; k < 3; ++k) out[3 + k] = (uint8_t)clamp8(a.m[3 * k] * c1 + t[k]);
        }
    }
}

// ---- egress ----

// crtfx_egress422_create admits only matrices whose accumulators stay in [0, 2^31): the lower clamp can never act, the shift is a logical one
// and the upper clamp (live: 256 at full range) is an unsigned minimum — the form of crtfx_egress.hip, for the reason given there.
__device__ __forceinline__ unsigned clamp8u(unsigned acc, int shift) { return min(acc >> shift, 255u); }
__device__ __forceinline__ unsigned luma(const Args& a, int r, int g, int b) { return clamp8u((unsigned)(a.m[0] * r + a.m[1] * g + a.m[2] * b + a.k[0]), SH); }
__device__ __forceinline__ unsigned chroma(const Args& a, int row, int r, int g, int b) {
    return clamp8u((unsigned)(a.m[3 * row] * r + a.m[3 * row + 1] * g + a.m[3 * row + 2] * b + a.k[row]), SH + 1);
}

// vec: one lane = one row of 8 columns, 24 RGB bytes in, 16 bytes out; general: one lane = one chroma sample (one macropixel), byte accesses.
template <int LAYOUT, int PATH>
__global__ __launch_bounds__(BLOCK) void k_egress_422(Args a) {
    const uint8_t* fsrc = a.src + (size_t)blockIdx.z * a.src_stride;
    uint8_t* fdst = a.dst + (size_t)blockIdx.z * a.dst_stride;
    const int idx = blockIdx.x * BLOCK + threadIdx.x;
    if (PATH == VEC) {
        const int nbx = a.w >> 3;
        if (idx >= a.h * nbx) return;
        const int y = idx / nbx, bx = idx - y * nbx;
        const U6 rgb = *reinterpret_cast<const U6*>(fsrc + (size_t)y * a.w * 3 + (size_t)bx * 24);
        unsigned yq[4][2], uq[4], vq[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {           // chroma sample q = columns 2q, 2q + 1
            int s[3] = {0, 0, 0};
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int p = 2 * q + e;
                int c[3];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const int b = 3 * p + ch;
                    c[ch] = (int)((rgb.v[b >> 2] >> (8 * (b & 3))) & 255u);
                    s[ch] += c[ch];
                }
                yq[q][e] = luma(a, c[0], c[1], c[2]);
            }
            uq[q] = chroma(a, 1, s[0], s[1], s[2]);
            vq[q] = chroma(a, 2, s[0], s[1], s[2]);
        }
        if (LAYOUT == CRTFX_422_YUV422P) {
            U2 yy{0u, 0u};
            unsigned up = 0u, vp = 0u;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned pair = (yq[q][0] | (yq[q][1] << 8)) << (16 * (q & 1));
                if (q < 2) yy.x |= pair; else yy.y |= pair;
                up |= uq[q] << (8 * q);
                vp |= vq[q] << (8 * q);
            }
            *reinterpret_cast<U2*>(fdst + (size_t)y * a.w + (size_t)bx * 8) = yy;
            uint8_t* cbase = fdst + (size_t)a.h * a.w;
            const size_t o = (size_t)y * a.cw + (size_t)bx * 4;
            *reinterpret_cast<unsigned*>(cbase + o) = up;
            *reinterpret_cast<unsigned*>(cbase + (size_t)a.h * a.cw + o) = vp;
        } else {
            using M = Mac<LAYOUT>;
            U4 mp;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                mp.v[q] = (yq[q][0] << (8 * M::Y0)) | (yq[q][1] << (8 * M::Y1)) | (uq[q] << (8 * M::U)) | (vq[q] << (8 * M::V));
            *reinterpret_cast<U4*>(fdst + (size_t)y * a.w * 2 + (size_t)bx * 16) = mp;
        }
    } else {
        if (idx >= a.h * a.cw) return;
        const int y = idx / a.cw, cx = idx - y * a.cw;
        const int x0 = 2 * cx;
        const bool right = x0 + 1 < a.w;
        const uint8_t* p0 = fsrc + ((size_t)y * a.w + x0) * 3;
        const uint8_t* p1 = right ? p0 + 3 : p0;
        const int r0 = p0[0], g0 = p0[1], b0 = p0[2];
        const int r1 = p1[0], g1 = p1[1], b1 = p1[2];
        const unsigned ya = luma(a, r0, g0, b0);
        const unsigned yb = luma(a, r1, g1, b1);                // at an odd edge: the row's last Y again, the pad byte of a packed row
        const unsigned u = chroma(a, 1, r0 + r1, g0 + g1, b0 + b1), v = chroma(a, 2, r0 + r1, g0 + g1, b0 + b1);
        if (LAYOUT == CRTFX_422_YUV422P) {
            uint8_t* yp = fdst + (size_t)y * a.w + x0;
            yp[0] = (uint8_t)ya;
            if (right) yp[1] = (uint8_t)yb;
            uint8_t* cbase = fdst + (size_t)a.h * a.w;
            const size_t o = (size_t)y * a.cw + cx;
            cbase[o] = (uint8_t)u;
            cbase[(size_t)a.h * a.cw + o] = (uint8_t)v;
        } else {
            using M = Mac<LAYOUT>;
            uint8_t* mp = fdst + ((size_t)y * a.cw + cx) * 4;
            mp[M::Y0] = (uint8_t)ya; mp[M::Y1] = (uint8_t)yb; mp[M::U] = (uint8_t)u; mp[M::V] = (uint8_t)v;
        }
    }
}

struct Plan : crtfx_stage::StagePlan { Args args{}; };         // what the two handle families share, told apart by `egress`

}  // namespace crtfx_422_impl

using namespace crtfx_422_impl;
using namespace crtfx_stage;

struct crtfx_unpack422 : Plan {};
struct crtfx_egress422 : Plan {};

namespace {

static_assert(SH == MATRIX_SH, "the row checks of crtfx_stage_host.h assume this matrix scale");
static_assert((int)CRTFX_UNPACK422_OPT_FORCE_GENERAL == (int)CRTFX_EGRESS422_OPT_FORCE_GENERAL, "one option number for both families");

const char* layout_name(int layout) { return layout == CRTFX_422_YUYV422 ? "yuyv422" : layout == CRTFX_422_UYVY422 ? "uyvy422" : "yuv422p"; }

template <int LAYOUT>
void launch_layout(const Plan* p, bool vec, dim3 grid, hipStream_t st, const Args& a) {
    if (p->egress) {
        if (vec) hipLaunchKernelGGL((k_egress_422<LAYOUT, VEC>), grid, dim3(BLOCK), 0, st, a);
        else hipLaunchKernelGGL((k_egress_422<LAYOUT, GENERAL>), grid, dim3(BLOCK), 0, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((k_unpack_422<LAYOUT, VEC>), grid, dim3(BLOCK), 0, st, a);
        else hipLaunchKernelGGL((k_unpack_422<LAYOUT, GENERAL>), grid, dim3(BLOCK), 0, st, a);
    }
}

struct Unit {
    static constexpr int block = BLOCK, force_option = CRTFX_UNPACK422_OPT_FORCE_GENERAL;
    static const char* name(bool egress) { return egress ? "egress422" : "unpack422"; }
    static void note_plan(Plan* p, bool vec, int frames) {
        const char* kernel = p->egress ? "egress422=k_egress_422" : "unpack422=k_unpack_422";
        snprintf(p->plan, sizeof p->plan, "%s<%s,%s>;frames=%d", kernel, layout_name(p->layout), vec ? "vec" : "general", frames);
    }
    static int check_alignment(Plan*, const void*, size_t, const void*, size_t) { return CRTFX_OK; }  // bytes: any base, any stride
    static int items(const Args& a, bool vec) { return vec ? a.h * (a.w >> 3) : a.h * a.cw; }          // at most 32767 * 16384
    static void launch(const Plan* p, bool vec, dim3 grid, hipStream_t st, const Args& a) {
        if (p->layout == CRTFX_422_YUYV422) launch_layout<CRTFX_422_YUYV422>(p, vec, grid, st, a);
        else if (p->layout == CRTFX_422_UYVY422) launch_layout<CRTFX_422_UYVY422>(p, vec, grid, st, a);
        else launch_layout<CRTFX_422_YUV422P>(p, vec, grid, st, a);
    }
};

template <class H>
int create(bool egress, int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, H** out_plan) {
    if (const int rc = begin_create(out_plan)) return rc;
    if (pix_fmt == CRTFX_PIX_F16)
        return fail<H>(nullptr, CRTFX_E_UNSUPPORTED, "only uint8 RGB frames are %s (the 4:2:2 stages have no half path)", egress ? "converted" : "written");
    const bool known = layout == CRTFX_422_YUV422P || layout == CRTFX_422_YUYV422 || layout == CRTFX_422_UYVY422;
    if (const int rc = check_create<H>(pix_fmt, CRTFX_PIX_U8, h, w, layout, known, m, off, 255)) return rc;
    long long k[3] = {off[0], off[1], off[2]};
    if (egress) {
        k[0] = ((long long)off[0] << SH) + (1LL << (SH - 1));
        k[1] = ((long long)off[1] << (SH + 1)) + (1LL << SH);
        k[2] = ((long long)off[2] << (SH + 1)) + (1LL << SH);
        if (!egress_row_fits(m, k[0], 255) || !egress_row_fits(m + 3, k[1], 510) || !egress_row_fits(m + 6, k[2], 510))
            return fail<H>(nullptr, CRTFX_E_INVALID, "the matrix lets an accumulator leave [0, 2^31)");
    } else if (!source_row_fits(m, 255) || !source_row_fits(m + 3, 255) || !source_row_fits(m + 6, 255)) {
        return fail<H>(nullptr, CRTFX_E_INVALID, "the matrix lets an accumulator leave int32");
    }
    H* p = nullptr;
    if (const int rc = new_plan(egress, device, layout, h, w, m, &p)) return rc;
    Args& a = p->args;
    a.cw = (w + 1) / 2;
    for (int i = 0; i < 3; ++i) a.k[i] = (int)k[i];
    p->frame_bytes = layout == CRTFX_422_YUV422P ? (size_t)h * w + 2 * (size_t)h * a.cw : 4 * (size_t)h * a.cw;
    p->rgb_bytes = (size_t)h * w * 3;
    Unit::note_plan(p, vec_fits(p, nullptr, 0, nullptr, 0, 1), 0);
    *out_plan = p;
    return CRTFX_OK;
}

}  // namespace

extern "C" {

const char* crtfx_unpack422_last_error(const crtfx_unpack422* p) { return p ? p->err.c_str() : create_err<crtfx_unpack422>().c_str(); }
int crtfx_unpack422_create(int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, crtfx_unpack422** out_plan) {
    return create(false, device, h, w, pix_fmt, layout, m, off, out_plan);
}
int crtfx_unpack422_destroy(crtfx_unpack422* p) { return destroy(p); }
size_t crtfx_unpack422_frame_bytes(const crtfx_unpack422* p) { return p ? p->frame_bytes : 0; }
int crtfx_unpack422_set_option(crtfx_unpack422* p, int option, int value) { return set_option<Unit>(p, option, value); }
int crtfx_unpack422_last_plan(crtfx_unpack422* p, char* buf, size_t n) { return last_plan(p, buf, n); }
int crtfx_unpack422_run(crtfx_unpack422* p, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream) {
    return run_frames<Unit>(p, src_base, src_stride_bytes, dst_base, dst_stride_bytes, n, stream);
}

const char* crtfx_egress422_last_error(const crtfx_egress422* p) { return p ? p->err.c_str() : create_err<crtfx_egress422>().c_str(); }
int crtfx_egress422_create(int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, crtfx_egress422** out_plan) {
    return create(true, device, h, w, pix_fmt, layout, m, off, out_plan);
}
int crtfx_egress422_destroy(crtfx_egress422* p) { return destroy(p); }
size_t crtfx_egress422_frame_bytes(const crtfx_egress422* p) { return p ? p->frame_bytes : 0; }
int crtfx_egress422_set_option(crtfx_egress422* p, int option, int value) { return set_option<Unit>(p, option, value); }
int crtfx_egress422_last_plan(crtfx_egress422* p, char* buf, size_t n) { return last_plan(p, buf, n); }
int crtfx_egress422_run(crtfx_egress422* p, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream) {
    return run_frames<Unit>(p, src_base, src_stride_bytes, dst_base, dst_stride_bytes, n, stream);
}

}  // extern "C"
