// crtfx_egress.hip — the egress stage of libcrtfx.so (include/crtfx_egress.h): finished uint8 RGB frames -> yuv420p / nv12 on the device.
// A translation unit of its own: it shares no kernel, table or handle with the effect chain or the ingest stage.  The host code around the kernels (checks, frame-group loop, error strings) is
// the skeleton of crtfx_stage_host.h: host templates only, so nothing is shared at run time either.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "crtfx_egress.h"
#include "crtfx_stage_host.h"

namespace crtfx_egress_impl {

constexpr int BLOCK = 256;
constexpr int SH = 16;                          // fractional bits of the matrix; a chroma sum of four samples carries two more

struct Args {
    const uint8_t* src; size_t src_stride;
    uint8_t* dst; size_t dst_stride;
    int h, w, ch, cw;
    int m[9];
    int ky, ku, kv;                             // (off << SH) + half for Y, (off << (SH + 2)) + half for U, V
};

// unsigned dwords at 4-byte alignment: the widest access the vec path's rule (crtfx_egress.h) guarantees
struct __attribute__((packed, aligned(4))) U2 { unsigned x, y; };
struct __attribute__((packed, aligned(4))) U6 { unsigned v[6]; };

// crtfx_egress_create admits only matrices whose accumulators stay in [0, 2^31): the lower clamp can never act, the shift is a logical one and
// the upper clamp (live: 256 at full range) is an unsigned minimum.  Written this way on purpose.  The signed form, clamp(acc >> 16, 0, 255) of
// two neighbouring samples packed into one word, is contracted to `v_ashr_pk_u8_i32 d, a, b, 16` with d = a's register, and the compiler then ORs
// the next sample into bits 16..23 as if the instruction had cleared them; on the MI355X they still held a's bits 16..23 — the first sample's
// own value — so every third and fourth byte of a word came out as (sample | first sample of the word).
__device__ __forceinline__ unsigned clamp8(unsigned acc, int shift) { return min(acc >> shift, 255u); }
__device__ __forceinline__ unsigned luma(const Args& a, int r, int g, int b) { return clamp8((unsigned)(a.m[0] * r + a.m[1] * g + a.m[2] * b + a.ky), SH); }
__device__ __forceinline__ unsigned chroma_u(const Args& a, int r, int g, int b) { return clamp8((unsigned)(a.m[3] * r + a.m[4] * g + a.m[5] * b + a.ku), SH + 2); }
__device__ __forceinline__ unsigned chroma_v(const Args& a, int r, int g, int b) { return clamp8((unsigned)(a.m[6] * r + a.m[7] * g + a.m[8] * b + a.kv), SH + 2); }

// vec path (w % 8 == 0, 4-byte-aligned frame bases): one lane = 2 rows x 8 columns of one frame; consecutive lanes, consecutive column
// blocks of a row pair, so a wave reads two contiguous runs of 64 x 24 bytes and writes contiguous runs of Y and chroma.
template <bool NV12>
__global__ __launch_bounds__(BLOCK) void k_egress_420_vec(Args a) {
    const int nbx = a.w >> 3;
    const int idx = blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= a.ch * nbx) return;
    const int cy = idx / nbx, bx = idx - cy * nbx;
    const int y0 = 2 * cy;
    const bool two = y0 + 1 < a.h;
    const uint8_t* fsrc = a.src + (size_t)blockIdx.z * a.src_stride;
    uint8_t* fdst = a.dst + (size_t)blockIdx.z * a.dst_stride;
    const size_t srow = (size_t)a.w * 3;
    const U6 r0 = *reinterpret_cast<const U6*>(fsrc + (size_t)y0 * srow + (size_t)bx * 24);
    const U6 r1 = *reinterpret_cast<const U6*>(fsrc + (size_t)(two ? y0 + 1 : y0) * srow + (size_t)bx * 24);

    unsigned ya[2] = {0u, 0u}, yb[2] = {0u, 0u}, up = 0u, vp = 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q) {               // chroma sample q = columns 2q, 2q + 1
        int s[3] = {0, 0, 0};
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int p = 2 * q + e;
            int c0[3], c1[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int b = 3 * p + c;
                c0[c] = (int)((r0.v[b >> 2] >> (8 * (b & 3))) & 255u);
                c1[c] = (int)((r1.v[b >> 2] >> (8 * (b & 3))) & 255u);
                s[c] += c0[c] + c1[c];
            }
            ya[p >> 2] |= (unsigned)luma(a, c0[0], c0[1], c0[2]) << (8 * (p & 3));
            yb[p >> 2] |= (unsigned)luma(a, c1[0], c1[1], c1[2]) << (8 * (p & 3));
        }
        up |= (unsigned)chroma_u(a, s[0], s[1], s[2]) << (8 * q);
        vp |= (unsigned)chroma_v(a, s[0], s[1], s[2]) << (8 * q);
    }
    uint8_t* yrow = fdst + (size_t)y0 * a.w + (size_t)bx * 8;
    *reinterpret_cast<U2*>(yrow) = U2{ya[0], ya[1]};
    if (two) *reinterpret_cast<U2*>(yrow + a.w) = U2{yb[0], yb[1]};
    uint8_t* cbase = fdst + (size_t)a.h * a.w;
    if (NV12) {
        // u0 v0 u1 v1 | u2 v2 u3 v3
        const unsigned lo = (up & 0xFFu) | ((vp & 0xFFu) << 8) | ((up & 0xFF00u) << 8) | ((vp & 0xFF00u) << 16);
        const unsigned hi = ((up >> 16) & 0xFFu) | (((vp >> 16) & 0xFFu) << 8) | ((up >> 8) & 0xFF0000u) | (vp & 0xFF000000u);
        *reinterpret_cast<U2*>(cbase + (size_t)cy * a.w + (size_t)bx * 8) = U2{lo, hi};
    } else {
        const size_t o = (size_t)cy * a.cw + (size_t)bx * 4;
        *reinterpret_cast<unsigned*>(cbase + o) = up;
        *reinterpret_cast<unsigned*>(cbase + (size_t)a.ch * a.cw + o) = vp;
    }
}

// general path: one lane = one chroma sample and the (up to) four luma samples under it; byte accesses only, any size and alignment
template <bool NV12>
__global__ __launch_bounds__(BLOCK) void k_egress_420_general(Args a) {
    const int idx = blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= a.ch * a.cw) return;
    const int cy = idx / a.cw, cx = idx - cy * a.cw;
    const int y0 = 2 * cy, x0 = 2 * cx;
    const bool right = x0 + 1 < a.w, below = y0 + 1 < a.h;
    const uint8_t* fsrc = a.src + (size_t)blockIdx.z * a.src_stride;
    uint8_t* fdst = a.dst + (size_t)blockIdx.z * a.dst_stride;
    const size_t srow = (size_t)a.w * 3;
    const uint8_t* p00 = fsrc + (size_t)y0 * srow + (size_t)x0 * 3;
    const uint8_t* p01 = right ? p00 + 3 : p00;
    const uint8_t* p10 = below ? p00 + srow : p00;
    const uint8_t* p11 = below ? p01 + srow : p01;
    const int r00 = p00[0], g00 = p00[1], b00 = p00[2];
    const int r01 = p01[0], g01 = p01[1], b01 = p01[2];
    const int r10 = p10[0], g10 = p10[1], b10 = p10[2];
    const int r11 = p11[0], g11 = p11[1], b11 = p11[2];
    uint8_t* y = fdst + (size_t)y0 * a.w + x0;
    y[0] = (uint8_t)luma(a, r00, g00, b00);
    if (right) y[1] = (uint8_t)luma(a, r01, g01, b01);
    if (below) {
        y[a.w] = (uint8_t)luma(a, r10, g10, b10);
        if (right) y[a.w + 1] = (uint8_t)luma(a, r11, g11, b11);
    }
    const int sr = r00 + r01 + r10 + r11, sg = g00 + g01 + g10 + g11, sb = b00 + b01 + b10 + b11;
    uint8_t* cbase = fdst + (size_t)a.h * a.w;
    const size_t o = (size_t)cy * a.cw + cx;
    if (NV12) {
        cbase[2 * o] = (uint8_t)chroma_u(a, sr, sg, sb);
        cbase[2 * o + 1] = (uint8_t)chroma_v(a, sr, sg, sb);
    } else {
        cbase[o] = (uint8_t)chroma_u(a, sr, sg, sb);
        cbase[(size_t)a.ch * a.cw + o] = (uint8_t)chroma_v(a, sr, sg, sb);
    }
}

}  // namespace crtfx_egress_impl

using namespace crtfx_egress_impl;
using namespace crtfx_stage;

struct crtfx_egress : StagePlan { Args args{}; };               // `egress` is always true

namespace {

struct Unit {
    static constexpr int block = BLOCK, force_option = CRTFX_EGRESS_OPT_FORCE_GENERAL;
    static const char* name(bool) { return "egress"; }
    static void note_plan(crtfx_egress* p, bool vec, int frames) {
        snprintf(p->plan, sizeof p->plan, "egress=k_egress_420<%s,%s>;frames=%d", p->layout == CRTFX_EGRESS_NV12 ? "nv12" : "yuv420p",
                 vec ? "vec" : "general", frames);
    }
    static int check_alignment(crtfx_egress*, const void*, size_t, const void*, size_t) { return CRTFX_OK; }    // bytes: any base, any stride
    static int items(const Args& a, bool vec) { return vec ? a.ch * (a.w >> 3) : a.ch * a.cw; }                // at most 16384 * 16384
    static void launch(const crtfx_egress* p, bool vec, dim3 grid, hipStream_t st, const Args& a) {
        const bool nv12 = p->layout == CRTFX_EGRESS_NV12;
        if (vec) {
            if (nv12) hipLaunchKernelGGL(k_egress_420_vec<true>, grid, dim3(BLOCK), 0, st, a);
            else hipLaunchKernelGGL(k_egress_420_vec<false>, grid, dim3(BLOCK), 0, st, a);
        } else {
            if (nv12) hipLaunchKernelGGL(k_egress_420_general<true>, grid, dim3(BLOCK), 0, st, a);
            else hipLaunchKernelGGL(k_egress_420_general<false>, grid, dim3(BLOCK), 0, st, a);
        }
    }
};

}  // namespace

extern "C" {

const char* crtfx_egress_last_error(const crtfx_egress* p) { return p ? p->err.c_str() : create_err<crtfx_egress>().c_str(); }

int crtfx_egress_create(int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, crtfx_egress** out_plan) {
    using H = crtfx_egress;
    if (const int rc = begin_create(out_plan)) return rc;
    if (pix_fmt == CRTFX_PIX_F16) return fail<H>(nullptr, CRTFX_E_UNSUPPORTED, "only uint8 RGB frames are converted (the egress stage takes finished frames)");
    if (const int rc = check_create<H>(pix_fmt, CRTFX_PIX_U8, h, w, layout, layout == CRTFX_EGRESS_YUV420P || layout == CRTFX_EGRESS_NV12, m, off, 255)) return rc;
    const long long ky = ((long long)off[0] << SH) + (1LL << (SH - 1));
    const long long ku = ((long long)off[1] << (SH + 2)) + (1LL << (SH + 1)), kv = ((long long)off[2] << (SH + 2)) + (1LL << (SH + 1));
    if (!egress_row_fits(m, ky, 255) || !egress_row_fits(m + 3, ku, 1020) || !egress_row_fits(m + 6, kv, 1020))
        return fail<H>(nullptr, CRTFX_E_INVALID, "the matrix lets an accumulator leave [0, 2^31)");
    H* p = nullptr;
    if (const int rc = new_plan(true, device, layout, h, w, m, &p)) return rc;
    Args& a = p->args;
    a.ch = (h + 1) / 2; a.cw = (w + 1) / 2;
    a.ky = (int)ky; a.ku = (int)ku; a.kv = (int)kv;
    p->frame_bytes = (size_t)h * w + 2 * (size_t)a.ch * a.cw;
    p->rgb_bytes = (size_t)h * w * 3;
    Unit::note_plan(p, vec_fits(p, nullptr, 0, nullptr, 0, 1), 0);
    *out_plan = p;
    return CRTFX_OK;
}

int crtfx_egress_destroy(crtfx_egress* p) { return destroy(p); }
size_t crtfx_egress_frame_bytes(const crtfx_egress* p) { return p ? p->frame_bytes : 0; }
int crtfx_egress_set_option(crtfx_egress* p, int option, int value) { return set_option<Unit>(p, option, value); }
int crtfx_egress_last_plan(crtfx_egress* p, char* buf, size_t n) { return last_plan(p, buf, n); }
int crtfx_egress_run(crtfx_egress* p, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream) {
    return run_frames<Unit>(p, src_base, src_stride_bytes, dst_base, dst_stride_bytes, n, stream);
}

}  // extern "C"
