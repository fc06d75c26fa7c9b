// crtfx_unpack.hip — the source stage of libcrtfx.so (include/crtfx_unpack.h): uint8 yuv420p / nv12 frames -> uint8 RGB on the device.
// A translation unit of its own: it shares no kernel, table or handle with the effect chain, the ingest stage or the egress stage.  The host code around the kernels (checks, frame-group loop, error strings) is
// the skeleton of crtfx_stage_host.h: host templates only, so nothing is shared at run time either.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "crtfx_unpack.h"
#include "crtfx_stage_host.h"

namespace crtfx_unpack_impl {

constexpr int BLOCK = 256;
constexpr int SH = 16;                          // fractional bits of the matrix

struct Args {
    const uint8_t* src; size_t src_stride;
    uint8_t* dst; size_t dst_stride;
    int h, w, ch, cw;
    int m[9];                                   // rows R, G, B over the columns Y, U, V
    int off[3];
};

// unsigned dwords at 4-byte alignment: the widest access the vec path's rule (crtfx_unpack.h) guarantees
struct __attribute__((packed, aligned(4))) U2 { unsigned x, y; };
struct __attribute__((packed, aligned(4))) U6 { unsigned v[6]; };

// clamp(acc >> SH, 0, 255) of a signed accumulator, written as: lower clamp on the accumulator (a negative quotient clamps to 0 whatever the
// shift does with the bits below it), a LOGICAL shift of the non-negative rest, an unsigned minimum.  On purpose: the signed form of two
// neighbouring samples packed into one word is contracted to v_ashr_pk_u8_i32, whose upper destination bits the MI355X keeps while the
// compiler assumes them cleared (see crtfx_egress.hip, where that gave wrong bytes).
__device__ __forceinline__ unsigned clamp8(int acc) { return min((unsigned)max(acc, 0) >> SH, 255u); }

// the chroma term of one chroma sample per output channel, rounding constant included: m[k][1] * d + m[k][2] * e + half
__device__ __forceinline__ void chroma_terms(const Args& a, int u, int v, int t[3]) {
    const int d = u - a.off[1], e = v - a.off[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = a.m[3 * k + 1] * d + a.m[3 * k + 2] * e + (1 << (SH - 1));
}

// vec path (w % 8 == 0, 4-byte-aligned frame bases): one lane = 2 rows x 8 columns of one frame; consecutive lanes, consecutive column
// blocks of a row pair, so a wave reads contiguous runs of Y and chroma and writes two contiguous runs of 64 x 24 bytes.
template <bool NV12>
__global__ __launch_bounds__(BLOCK) void k_unpack_420_vec(Args a) {
    const int nbx = a.w >> 3;
    const int idx = blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= a.ch * nbx) return;
    const int cy = idx / nbx, bx = idx - cy * nbx;
    const int y0 = 2 * cy;
    const bool two = y0 + 1 < a.h;
    const uint8_t* fsrc = a.src + (size_t)blockIdx.z * a.src_stride;
    uint8_t* fdst = a.dst + (size_t)blockIdx.z * a.dst_stride;
    const uint8_t* yrow = fsrc + (size_t)y0 * a.w + (size_t)bx * 8;
    const U2 ya = *reinterpret_cast<const U2*>(yrow);
    const U2 yb = *reinterpret_cast<const U2*>(two ? yrow + a.w : yrow);
    const uint8_t* cbase = fsrc + (size_t)a.h * a.w;
    unsigned up, vp;                            // u0 u1 u2 u3, v0 v1 v2 v3
    if (NV12) {
        const U2 uv = *reinterpret_cast<const U2*>(cbase + (size_t)cy * a.w + (size_t)bx * 8);          // u0 v0 u1 v1 | u2 v2 u3 v3
        up = (uv.x & 0xFFu) | ((uv.x >> 8) & 0xFF00u) | ((uv.y & 0xFFu) << 16) | ((uv.y & 0xFF0000u) << 8);
        vp = ((uv.x >> 8) & 0xFFu) | ((uv.x >> 16) & 0xFF00u) | ((uv.y & 0xFF00u) << 8) | (uv.y & 0xFF000000u);
    } else {
        const size_t o = (size_t)cy * a.cw + (size_t)bx * 4;
        up = *reinterpret_cast<const unsigned*>(cbase + o);
        vp = *reinterpret_cast<const unsigned*>(cbase + (size_t)a.ch * a.cw + o);
    }
    const unsigned yw[2][2] = {{ya.x, ya.y}, {yb.x, yb.y}};
    U6 o0, o1;
#pragma unroll
    for (int i = 0; i < 6; ++i) { o0.v[i] = 0u; o1.v[i] = 0u; }
#pragma unroll
    for (int q = 0; q < 4; ++q) {               // chroma sample q = columns 2q, 2q + 1
        int t[3];
        chroma_terms(a, (int)((up >> (8 * q)) & 255u), (int)((vp >> (8 * q)) & 255u), t);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int p = 2 * q + e;
            const int c0 = (int)((yw[0][p >> 2] >> (8 * (p & 3))) & 255u) - a.off[0];
            const int c1 = (int)((yw[1][p >> 2] >> (8 * (p & 3))) & 255u) - a.off[0];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int b = 3 * p + k;
                o0.v[b >> 2] |= clamp8(a.m[3 * k] * c0 + t[k]) << (8 * (b & 3));
                o1.v[b >> 2] |= clamp8(a.m[3 * k] * c1 + t[k]) << (8 * (b & 3));
            }
        }
    }
    const size_t drow = (size_t)a.w * 3;
    uint8_t* out = fdst + (size_t)y0 * drow + (size_t)bx * 24;
    *reinterpret_cast<U6*>(out) = o0;
    if (two) *reinterpret_cast<U6*>(out + drow) = o1;
}

// general path: one lane = one chroma sample and the (up to) four pixels under it; byte accesses only, any size and alignment
template <bool NV12>
__global__ __launch_bounds__(BLOCK) void k_unpack_420_general(Args a) {
    const int idx = blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= a.ch * a.cw) return;
    const int cy = idx / a.cw, cx = idx - cy * a.cw;
    const int y0 = 2 * cy, x0 = 2 * cx;
    const bool right = x0 + 1 < a.w, below = y0 + 1 < a.h;
    const uint8_t* fsrc = a.src + (size_t)blockIdx.z * a.src_stride;
    uint8_t* fdst = a.dst + (size_t)blockIdx.z * a.dst_stride;
    const uint8_t* cbase = fsrc + (size_t)a.h * a.w;
    const size_t o = (size_t)cy * a.cw + cx;
    int u, v;
    if (NV12) {
        u = cbase[2 * o]; v = cbase[2 * o + 1];
    } else {
        u = cbase[o]; v = cbase[(size_t)a.ch * a.cw + o];
    }
    int t[3];
    chroma_terms(a, u, v, t);
    const size_t drow = (size_t)a.w * 3;
    const uint8_t* yp = fsrc + (size_t)y0 * a.w + x0;
    uint8_t* out = fdst + (size_t)y0 * drow + (size_t)x0 * 3;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (r == 1 && !below) break;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            if (e == 1 && !right) break;
            const int c = (int)yp[(size_t)r * a.w + e] - a.off[0];
#pragma unroll
            for (int k = 0; k < 3; ++k) out[(size_t)r * drow + 3 * e + k] = (uint8_t)clamp8(a.m[3 * k] * c + t[k]);
        }
    }
}

}  // namespace crtfx_unpack_impl

using namespace crtfx_unpack_impl;
using namespace crtfx_stage;

struct crtfx_unpack : StagePlan { Args args{}; };               // `egress` stays false

namespace {

static_assert(SH == MATRIX_SH, "the row checks of crtfx_stage_host.h assume this matrix scale");

struct Unit {
    static constexpr int block = BLOCK, force_option = CRTFX_UNPACK_OPT_FORCE_GENERAL;
    static const char* name(bool) { return "unpack"; }
    static void note_plan(crtfx_unpack* p, bool vec, int frames) {
        snprintf(p->plan, sizeof p->plan, "unpack=k_unpack_420<%s,%s>;frames=%d", p->layout == CRTFX_UNPACK_NV12 ? "nv12" : "yuv420p",
                 vec ? "vec" : "general", frames);
    }
    static int check_alignment(crtfx_unpack*, const void*, size_t, const void*, size_t) { return CRTFX_OK; }    // bytes: any base, any stride
    static int items(const Args& a, bool vec) { return vec ? a.ch * (a.w >> 3) : a.ch * a.cw; }                // at most 16384 * 16384
    static void launch(const crtfx_unpack* p, bool vec, dim3 grid, hipStream_t st, const Args& a) {
        const bool nv12 = p->layout == CRTFX_UNPACK_NV12;
        if (vec) {
            if (nv12) hipLaunchKernelGGL(k_unpack_420_vec<true>, grid, dim3(BLOCK), 0, st, a);
            else hipLaunchKernelGGL(k_unpack_420_vec<false>, grid, dim3(BLOCK), 0, st, a);
        } else {
            if (nv12) hipLaunchKernelGGL(k_unpack_420_general<true>, grid, dim3(BLOCK), 0, st, a);
            else hipLaunchKernelGGL(k_unpack_420_general<false>, grid, dim3(BLOCK), 0, st, a);
        }
    }
};

}  // namespace

extern "C" {

const char* crtfx_unpack_last_error(const crtfx_unpack* p) { return p ? p->err.c_str() : create_err<crtfx_unpack>().c_str(); }

int crtfx_unpack_create(int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, crtfx_unpack** out_plan) {
    using H = crtfx_unpack;
    if (const int rc = begin_create(out_plan)) return rc;
    if (pix_fmt == CRTFX_PIX_F16) return fail<H>(nullptr, CRTFX_E_UNSUPPORTED, "only uint8 RGB frames are written (the source stage feeds the chain's uint8 input)");
    if (const int rc = check_create<H>(pix_fmt, CRTFX_PIX_U8, h, w, layout, layout == CRTFX_UNPACK_YUV420P || layout == CRTFX_UNPACK_NV12, m, off, 255)) return rc;
    if (!source_row_fits(m, 255) || !source_row_fits(m + 3, 255) || !source_row_fits(m + 6, 255))
        return fail<H>(nullptr, CRTFX_E_INVALID, "the matrix lets an accumulator leave int32");
    H* p = nullptr;
    if (const int rc = new_plan(false, device, layout, h, w, m, &p)) return rc;
    Args& a = p->args;
    a.ch = (h + 1) / 2; a.cw = (w + 1) / 2;
    for (int i = 0; i < 3; ++i) a.off[i] = off[i];
    p->frame_bytes = (size_t)h * w + 2 * (size_t)a.ch * a.cw;
    p->rgb_bytes = (size_t)h * w * 3;
    Unit::note_plan(p, vec_fits(p, nullptr, 0, nullptr, 0, 1), 0);
    *out_plan = p;
    return CRTFX_OK;
}

int crtfx_unpack_destroy(crtfx_unpack* p) { return destroy(p); }
size_t crtfx_unpack_frame_bytes(const crtfx_unpack* p) { return p ? p->frame_bytes : 0; }
int crtfx_unpack_set_option(crtfx_unpack* p, int option, int value) { return set_option<Unit>(p, option, value); }
int crtfx_unpack_last_plan(crtfx_unpack* p, char* buf, size_t n) { return last_plan(p, buf, n); }
int crtfx_unpack_run(crtfx_unpack* p, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream) {
    return run_frames<Unit>(p, src_base, src_stride_bytes, dst_base, dst_stride_bytes, n, stream);
}

}  // extern "C"
