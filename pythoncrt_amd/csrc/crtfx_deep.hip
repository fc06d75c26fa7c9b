// crtfx_deep.hip — the 10-bit pair of libcrtfx.so (include/crtfx_deep.h): yuv420p10le / p010le frames -> half RGB in front of a half chain,
// half RGB -> yuv420p10le / p010le behind it.  A translation unit of its own: it shares no kernel, table or handle with the effect chain,
// the ingest stage or the 8-bit source and egress stages.  The host code around the kernels (checks, frame-group loop, error strings) is
// the skeleton of crtfx_stage_host.h: host templates only, so nothing is shared at run time either.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "crtfx_deep.h"
#include "crtfx_stage_host.h"

namespace crtfx_deep_impl {

constexpr int BLOCK = 256;
constexpr int SH = 16;                          // fractional bits of the matrix; a chroma sum of four samples carries two more
constexpr unsigned QMAX = 1020u;                // the largest quarter code: 255.0 on the half scale
constexpr unsigned CMAX = 1023u;                // the largest 10-bit code

struct Args {
    const uint8_t* src; size_t src_stride;
    uint8_t* dst; size_t dst_stride;
    int h, w, ch, cw;
    int m[9];
    int k[3];                                   // source: off.  egress: (off0 << SH) + half, (off << (SH + 2)) + half for U, V
};

// unsigned dwords at 4-byte alignment: the widest access the vec path's rule (crtfx_deep.h) guarantees
struct __attribute__((packed, aligned(4))) U2 { unsigned v[2]; };
struct __attribute__((packed, aligned(4))) U4 { unsigned v[4]; };
struct __attribute__((packed, aligned(4))) U12 { unsigned v[12]; };

// the 10-bit sample of a 16-bit word (bits outside the sample are ignored) and the word of a sample
template <bool P010> __device__ __forceinline__ int sample(unsigned word16) { return (int)(P010 ? word16 >> 6 : word16 & CMAX); }
template <bool P010> __device__ __forceinline__ int sample_lo(unsigned dword) { return sample<P010>(dword & 0xFFFFu); }
template <bool P010> __device__ __forceinline__ int sample_hi(unsigned dword) { return sample<P010>(dword >> 16); }
template <bool P010> __device__ __forceinline__ unsigned word(unsigned v) { return P010 ? v << 6 : v; }

// ---- source: 10-bit 4:2:0 -> half RGB --------------------------------------------------------------------------------------------------

// clamp(acc >> SH, 0, 1020) of a signed accumulator in the form of the 8-bit kernels (crtfx_unpack.hip says why): lower clamp on the
// accumulator, a LOGICAL shift of the non-negative rest, an unsigned minimum.
__device__ __forceinline__ unsigned quarter(int acc) { return min((unsigned)max(acc, 0) >> SH, QMAX); }

// the half bit pattern of quarter code q, q / 4 on the 0..255 scale: exact, every quarter code is a half (no rounding occurs)
__device__ __forceinline__ unsigned half_bits(unsigned q) { return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)((float)q * 0.25f)); }

// the chroma term of one chroma sample per output channel, rounding constant included: m[k][1] * d + m[k][2] * e + half
__device__ __forceinline__ void chroma_terms(const Args& a, int u, int v, int t[3]) {
    const int d = u - a.k[1], e = v - a.k[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = a.m[3 * k + 1] * d + a.m[3 * k + 2] * e + (1 << (SH - 1));
}

// vec path (w % 8 == 0, 4-byte-aligned frame bases): one lane = 2 rows x 8 columns of one frame; consecutive lanes, consecutive column
// blocks of a row pair, so a wave reads contiguous runs of Y (64 x 16 bytes per row) and chroma and writes two contiguous runs of 64 x 48 bytes.
template <bool P010>
__global__ __launch_bounds__(BLOCK) void k_unpack10_420_vec(Args a) {
    const int nbx = a.w >> 3;
    const int idx = blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= a.ch * nbx) return;
    const int cy = idx / nbx, bx = idx - cy * nbx;
    const int y0 = 2 * cy;
    const bool two = y0 + 1 < a.h;
    const uint8_t* fsrc = a.src + (size_t)blockIdx.z * a.src_stride;
    uint8_t* fdst = a.dst + (size_t)blockIdx.z * a.dst_stride;
    const size_t yrow_b = (size_t)a.w * 2;
    const uint8_t* yrow = fsrc + (size_t)y0 * yrow_b + (size_t)bx * 16;
    const U4 ya = *reinterpret_cast<const U4*>(yrow);
    const U4 yb = *reinterpret_cast<const U4*>(two ? yrow + yrow_b : yrow);
    const uint8_t* cbase = fsrc + (size_t)a.h * yrow_b;
    int u[4], v[4];
    if (P010) {                                 // u0 v0 | u1 v1 | u2 v2 | u3 v3: one chroma sample per dword
        const U4 uv = *reinterpret_cast<const U4*>(cbase + (size_t)cy * yrow_b + (size_t)bx * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) { u[q] = sample_lo<P010>(uv.v[q]); v[q] = sample_hi<P010>(uv.v[q]); }
    } else {
        const size_t o = ((size_t)cy * a.cw + (size_t)bx * 4) * 2;
        const U2 up = *reinterpret_cast<const U2*>(cbase + o);
        const U2 vp = *reinterpret_cast<const U2*>(cbase + (size_t)a.ch * a.cw * 2 + o);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            u[q] = (q & 1) ? sample_hi<P010>(up.v[q >> 1]) : sample_lo<P010>(up.v[q >> 1]);
            v[q] = (q & 1) ? sample_hi<P010>(vp.v[q >> 1]) : sample_lo<P010>(vp.v[q >> 1]);
        }
    }
    unsigned h0[24], h1[24];                    // the half patterns of the two rows, 8 pixels x (R, G, B)
#pragma unroll
    for (int q = 0; q < 4; ++q) {               // chroma sample q = columns 2q, 2q + 1 = the two halves of Y dword q
        int t[3];
        chroma_terms(a, u[q], v[q], t);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int c0 = (e ? sample_hi<P010>(ya.v[q]) : sample_lo<P010>(ya.v[q])) - a.k[0];
            const int c1 = (e ? sample_hi<P010>(yb.v[q]) : sample_lo<P010>(yb.v[q])) - a.k[0];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                h0[3 * (2 * q + e) + k] = half_bits(quarter(a.m[3 * k] * c0 + t[k]));
                h1[3 * (2 * q + e) + k] = half_bits(quarter(a.m[3 * k] * c1 + t[k]));
            }
        }
    }
    U12 o0, o1;
#pragma unroll
    for (int i = 0; i < 12; ++i) { o0.v[i] = h0[2 * i] | (h0[2 * i + 1] << 16); o1.v[i] = h1[2 * i] | (h1[2 * i + 1] << 16); }
    const size_t drow = (size_t)a.w * 6;
    uint8_t* out = fdst + (size_t)y0 * drow + (size_t)bx * 48;
    *reinterpret_cast<U12*>(out) = o0;
    if (two) *reinterpret_cast<U12*>(out + drow) = o1;
}

// general path: one lane = one chroma sample and the (up to) four pixels under it; 16-bit accesses only, any size, 2-byte-aligned bases
template <bool P010>
__global__ __launch_bounds__(BLOCK) void k_unpack10_420_general(Args a) {
    const int idx = blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= a.ch * a.cw) return;
    const int cy = idx / a.cw, cx = idx - cy * a.cw;
    const int y0 = 2 * cy, x0 = 2 * cx;
    const bool right = x0 + 1 < a.w, below = y0 + 1 < a.h;
    const uint16_t* fsrc = reinterpret_cast<const uint16_t*>(a.src + (size_t)blockIdx.z * a.src_stride);
    uint16_t* fdst = reinterpret_cast<uint16_t*>(a.dst + (size_t)blockIdx.z * a.dst_stride);
    const uint16_t* cbase = fsrc + (size_t)a.h * a.w;
    const size_t o = (size_t)cy * a.cw + cx;
    int u, v;
    if (P010) {
        u = sample<P010>(cbase[2 * o]); v = sample<P010>(cbase[2 * o + 1]);
    } else {
        u = sample<P010>(cbase[o]); v = sample<P010>(cbase[(size_t)a.ch * a.cw + o]);
    }
    int t[3];
    chroma_terms(a, u, v, t);
    const size_t drow = (size_t)a.w * 3;
    const uint16_t* yp = fsrc + (size_t)y0 * a.w + x0;
    uint16_t* out = fdst + (size_t)y0 * drow + (size_t)x0 * 3;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (r == 1 && !below) break;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            if (e == 1 && !right) break;
            const int c = sample<P010>(yp[(size_t)r * a.w + e]) - a.k[0];
#pragma unroll
            for (int k = 0; k < 3; ++k) out[(size_t)r * drow + 3 * e + k] = (uint16_t)half_bits(quarter(a.m[3 * k] * c + t[k]));
        }
    }
}

// ---- egress: half RGB -> 10-bit 4:2:0 --------------------------------------------------------------------------------------------------

// the quarter code of a half bit pattern: rint_to_even(min(max(4 f, 0), 1020)), NaN -> 0.  The half -> float conversion and 4 f are exact;
// the comparisons are written out so that a NaN (either kind) fails `> 0` and takes the 0, as -0, negatives and -inf do; +inf takes 1020.
__device__ __forceinline__ int quantise(unsigned bits16) {
    float t = 4.0f * (float)__builtin_bit_cast(_Float16, (unsigned short)bits16);
    t = t > 0.0f ? t : 0.0f;
    t = t < 1020.0f ? t : 1020.0f;
    return (int)rintf(t);
}

// crtfx_egress10_create admits only matrices whose accumulators stay in [0, 2^31): the lower clamp can never act, the shift is a logical one
// and the upper clamp is an unsigned minimum (the form of crtfx_egress.hip, for the reason given there).
__device__ __forceinline__ unsigned clamp10(unsigned acc, int shift) { return min(acc >> shift, CMAX); }
__device__ __forceinline__ unsigned luma(const Args& a, const int q[3]) { return clamp10((unsigned)(a.m[0] * q[0] + a.m[1] * q[1] + a.m[2] * q[2] + a.k[0]), SH); }
__device__ __forceinline__ unsigned chroma(const Args& a, int row, const int s[3]) {
    return clamp10((unsigned)(a.m[3 * row] * s[0] + a.m[3 * row + 1] * s[1] + a.m[3 * row + 2] * s[2] + a.k[row]), SH + 2);
}

// vec path: one lane = 2 rows x 8 columns of one frame; a wave reads two contiguous runs of 64 x 48 bytes and writes contiguous runs of
// Y (64 x 16 bytes per row) and chroma.
template <bool P010>
__global__ __launch_bounds__(BLOCK) void k_egress10_420_vec(Args a) {
    const int nbx = a.w >> 3;
    const int idx = blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= a.ch * nbx) return;
    const int cy = idx / nbx, bx = idx - cy * nbx;
    const int y0 = 2 * cy;
    const bool two = y0 + 1 < a.h;
    const uint8_t* fsrc = a.src + (size_t)blockIdx.z * a.src_stride;
    uint8_t* fdst = a.dst + (size_t)blockIdx.z * a.dst_stride;
    const size_t srow = (size_t)a.w * 6;
    const U12 r0 = *reinterpret_cast<const U12*>(fsrc + (size_t)y0 * srow + (size_t)bx * 48);
    const U12 r1 = *reinterpret_cast<const U12*>(fsrc + (size_t)(two ? y0 + 1 : y0) * srow + (size_t)bx * 48);
    U4 ya, yb;
    unsigned uq[4], vq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {               // chroma sample q = columns 2q, 2q + 1 = halves 6q .. 6q + 5 = dwords 3q .. 3q + 2
        int p0[2][3], p1[2][3], s[3];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const unsigned d0 = r0.v[3 * q + (j >> 1)], d1 = r1.v[3 * q + (j >> 1)];
            p0[j / 3][j % 3] = quantise((j & 1) ? d0 >> 16 : d0 & 0xFFFFu);
            p1[j / 3][j % 3] = quantise((j & 1) ? d1 >> 16 : d1 & 0xFFFFu);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] = p0[0][c] + p0[1][c] + p1[0][c] + p1[1][c];
        ya.v[q] = word<P010>(luma(a, p0[0])) | (word<P010>(luma(a, p0[1])) << 16);
        yb.v[q] = word<P010>(luma(a, p1[0])) | (word<P010>(luma(a, p1[1])) << 16);
        uq[q] = word<P010>(chroma(a, 1, s));
        vq[q] = word<P010>(chroma(a, 2, s));
    }
    const size_t yrow_b = (size_t)a.w * 2;
    uint8_t* yrow = fdst + (size_t)y0 * yrow_b + (size_t)bx * 16;
    *reinterpret_cast<U4*>(yrow) = ya;
    if (two) *reinterpret_cast<U4*>(yrow + yrow_b) = yb;
    uint8_t* cbase = fdst + (size_t)a.h * yrow_b;
    if (P010) {
        U4 uv;
#pragma unroll
        for (int q = 0; q < 4; ++q) uv.v[q] = uq[q] | (vq[q] << 16);
        *reinterpret_cast<U4*>(cbase + (size_t)cy * yrow_b + (size_t)bx * 16) = uv;
    } else {
        const size_t o = ((size_t)cy * a.cw + (size_t)bx * 4) * 2;
        U2 up, vp;
#pragma unroll
        for (int i = 0; i < 2; ++i) { up.v[i] = uq[2 * i] | (uq[2 * i + 1] << 16); vp.v[i] = vq[2 * i] | (vq[2 * i + 1] << 16); }
        *reinterpret_cast<U2*>(cbase + o) = up;
        *reinterpret_cast<U2*>(cbase + (size_t)a.ch * a.cw * 2 + o) = vp;
    }
}

// general path: one lane = one chroma sample and the (up to) four luma samples under it; 16-bit accesses only
template <bool P010>
__global__ __launch_bounds__(BLOCK) void k_egress10_420_general(Args a) {
    const int idx = blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= a.ch * a.cw) return;
    const int cy = idx / a.cw, cx = idx - cy * a.cw;
    const int y0 = 2 * cy, x0 = 2 * cx;
    const bool right = x0 + 1 < a.w, below = y0 + 1 < a.h;
    const uint16_t* fsrc = reinterpret_cast<const uint16_t*>(a.src + (size_t)blockIdx.z * a.src_stride);
    uint16_t* fdst = reinterpret_cast<uint16_t*>(a.dst + (size_t)blockIdx.z * a.dst_stride);
    const size_t srow = (size_t)a.w * 3;
    const uint16_t* p00 = fsrc + (size_t)y0 * srow + (size_t)x0 * 3;
    const uint16_t* p01 = right ? p00 + 3 : p00;
    const uint16_t* p10 = below ? p00 + srow : p00;
    const uint16_t* p11 = below ? p01 + srow : p01;
    int q00[3], q01[3], q10[3], q11[3], s[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        q00[c] = quantise(p00[c]); q01[c] = quantise(p01[c]); q10[c] = quantise(p10[c]); q11[c] = quantise(p11[c]);
        s[c] = q00[c] + q01[c] + q10[c] + q11[c];
    }
    uint16_t* y = fdst + (size_t)y0 * a.w + x0;
    y[0] = (uint16_t)word<P010>(luma(a, q00));
    if (right) y[1] = (uint16_t)word<P010>(luma(a, q01));
    if (below) {
        y[a.w] = (uint16_t)word<P010>(luma(a, q10));
        if (right) y[a.w + 1] = (uint16_t)word<P010>(luma(a, q11));
    }
    uint16_t* cbase = fdst + (size_t)a.h * a.w;
    const size_t o = (size_t)cy * a.cw + cx;
    if (P010) {
        cbase[2 * o] = (uint16_t)word<P010>(chroma(a, 1, s));
        cbase[2 * o + 1] = (uint16_t)word<P010>(chroma(a, 2, s));
    } else {
        cbase[o] = (uint16_t)word<P010>(chroma(a, 1, s));
        cbase[(size_t)a.ch * a.cw + o] = (uint16_t)word<P010>(chroma(a, 2, s));
    }
}

struct Plan : crtfx_stage::StagePlan { Args args{}; };         // what the two handle families share, told apart by `egress`

}  // namespace crtfx_deep_impl

using namespace crtfx_deep_impl;
using namespace crtfx_stage;

struct crtfx_unpack10 : Plan {};
struct crtfx_egress10 : Plan {};

namespace {

static_assert(SH == MATRIX_SH, "the row checks of crtfx_stage_host.h assume this matrix scale");
static_assert((int)CRTFX_UNPACK10_OPT_FORCE_GENERAL == (int)CRTFX_EGRESS10_OPT_FORCE_GENERAL, "one option number for both families");

template <bool P010>
void launch_layout(const Plan* p, bool vec, dim3 grid, hipStream_t st, const Args& a) {
    if (p->egress) {
        if (vec) hipLaunchKernelGGL(k_egress10_420_vec<P010>, grid, dim3(BLOCK), 0, st, a);
        else hipLaunchKernelGGL(k_egress10_420_general<P010>, grid, dim3(BLOCK), 0, st, a);
    } else {
        if (vec) hipLaunchKernelGGL(k_unpack10_420_vec<P010>, grid, dim3(BLOCK), 0, st, a);
        else hipLaunchKernelGGL(k_unpack10_420_general<P010>, grid, dim3(BLOCK), 0, st, a);
    }
}

struct Unit {
    static constexpr int block = BLOCK, force_option = CRTFX_UNPACK10_OPT_FORCE_GENERAL;
    static const char* name(bool egress) { return egress ? "egress10" : "unpack10"; }
    static void note_plan(Plan* p, bool vec, int frames) {
        const char* kernel = p->egress ? "egress10=k_egress10_420" : "unpack10=k_unpack10_420";
        snprintf(p->plan, sizeof p->plan, "%s<%s,%s>;frames=%d", kernel, p->layout == CRTFX_DEEP_P010LE ? "p010le" : "yuv420p10le", vec ? "vec" : "general", frames);
    }
    static int check_alignment(Plan* p, const void* src_base, size_t src_stride_bytes, const void* dst_base, size_t dst_stride_bytes) {
        if ((reinterpret_cast<uintptr_t>(src_base) | reinterpret_cast<uintptr_t>(dst_base) | src_stride_bytes | dst_stride_bytes) & 1u)
            return fail(p, CRTFX_E_INVALID, "an odd frame base or stride: 16-bit samples need 2-byte alignment");
        return CRTFX_OK;
    }
    static int items(const Args& a, bool vec) { return vec ? a.ch * (a.w >> 3) : a.ch * a.cw; }       // at most 16384 * 16384
    static void launch(const Plan* p, bool vec, dim3 grid, hipStream_t st, const Args& a) {
        if (p->layout == CRTFX_DEEP_P010LE) launch_layout<true>(p, vec, grid, st, a);
        else launch_layout<false>(p, vec, grid, st, a);
    }
};

template <class H>
int create(bool egress, int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, H** out_plan) {
    if (const int rc = begin_create(out_plan)) return rc;
    if (pix_fmt == CRTFX_PIX_U8)
        return fail<H>(nullptr, CRTFX_E_UNSUPPORTED, "only half RGB frames are %s (uint8 frames take the 8-bit %s stage)", egress ? "converted" : "written", egress ? "egress" : "source");
    if (const int rc = check_create<H>(pix_fmt, CRTFX_PIX_F16, h, w, layout, layout == CRTFX_DEEP_YUV420P10LE || layout == CRTFX_DEEP_P010LE, m, off, CMAX)) return rc;
    long long k[3] = {off[0], off[1], off[2]};
    if (egress) {
        k[0] = ((long long)off[0] << SH) + (1LL << (SH - 1));
        k[1] = ((long long)off[1] << (SH + 2)) + (1LL << (SH + 1));
        k[2] = ((long long)off[2] << (SH + 2)) + (1LL << (SH + 1));
        if (!egress_row_fits(m, k[0], 1020) || !egress_row_fits(m + 3, k[1], 4080) || !egress_row_fits(m + 6, k[2], 4080))
            return fail<H>(nullptr, CRTFX_E_INVALID, "the matrix lets an accumulator leave [0, 2^31)");
    } else if (!source_row_fits(m, CMAX) || !source_row_fits(m + 3, CMAX) || !source_row_fits(m + 6, CMAX)) {
        return fail<H>(nullptr, CRTFX_E_INVALID, "the matrix lets an accumulator leave int32");
    }
    H* p = nullptr;
    if (const int rc = new_plan(egress, device, layout, h, w, m, &p)) return rc;
    Args& a = p->args;
    a.ch = (h + 1) / 2; a.cw = (w + 1) / 2;
    for (int i = 0; i < 3; ++i) a.k[i] = (int)k[i];
    p->frame_bytes = 2 * ((size_t)h * w + 2 * (size_t)a.ch * a.cw);
    p->rgb_bytes = (size_t)h * w * 6;
    Unit::note_plan(p, vec_fits(p, nullptr, 0, nullptr, 0, 1), 0);
    *out_plan = p;
    return CRTFX_OK;
}

}  // namespace

extern "C" {

const char* crtfx_unpack10_last_error(const crtfx_unpack10* p) { return p ? p->err.c_str() : create_err<crtfx_unpack10>().c_str(); }
int crtfx_unpack10_create(int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, crtfx_unpack10** out_plan) {
    return create(false, device, h, w, pix_fmt, layout, m, off, out_plan);
}
int crtfx_unpack10_destroy(crtfx_unpack10* p) { return destroy(p); }
size_t crtfx_unpack10_frame_bytes(const crtfx_unpack10* p) { return p ? p->frame_bytes : 0; }
int crtfx_unpack10_set_option(crtfx_unpack10* p, int option, int value) { return set_option<Unit>(p, option, value); }
int crtfx_unpack10_last_plan(crtfx_unpack10* p, char* buf, size_t n) { return last_plan(p, buf, n); }
int crtfx_unpack10_run(crtfx_unpack10* p, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream) {
    return run_frames<Unit>(p, src_base, src_stride_bytes, dst_base, dst_stride_bytes, n, stream);
}

const char* crtfx_egress10_last_error(const crtfx_egress10* p) { return p ? p->err.c_str() : create_err<crtfx_egress10>().c_str(); }
int crtfx_egress10_create(int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, crtfx_egress10** out_plan) {
    return create(true, device, h, w, pix_fmt, layout, m, off, out_plan);
}
int crtfx_egress10_destroy(crtfx_egress10* p) { return destroy(p); }
size_t crtfx_egress10_frame_bytes(const crtfx_egress10* p) { return p ? p->frame_bytes : 0; }
int crtfx_egress10_set_option(crtfx_egress10* p, int option, int value) { return set_option<Unit>(p, option, value); }
int crtfx_egress10_last_plan(crtfx_egress10* p, char* buf, size_t n) { return last_plan(p, buf, n); }
int crtfx_egress10_run(crtfx_egress10* p, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream) {
    return run_frames<Unit>(p, src_base, src_stride_bytes, dst_base, dst_stride_bytes, n, stream);
}

}  // extern "C"
