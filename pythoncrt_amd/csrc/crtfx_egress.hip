// crtfx_egress.hip — the egress stage of libcrtfx.so (include/crtfx_egress.h): finished uint8 RGB frames -> yuv420p / nv12 on the device.
// A translation unit of its own: it shares no kernel, table or handle with the effect chain or the ingest stage.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>

#include "crtfx_egress.h"

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

struct crtfx_egress {
    int device = 0;
    int layout = CRTFX_EGRESS_YUV420P;
    Args args{};                        // launch constants (frame pointers filled per run)
    size_t frame_bytes = 0;
    bool force_general = false;
    char plan[128] = "";
    std::string err;
};

namespace {

thread_local std::string g_create_err;

int fail(crtfx_egress* p, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (p) p->err = buf; else g_create_err = buf;
    return code;
}

struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) { err = hipSetDevice(dev); switched = err == hipSuccess; }
    }
    ~DeviceGuard() { if (switched && prev >= 0) (void)hipSetDevice(prev); }
};

// the accumulator of one row stays in [0, 2^31) for every input: constant + (negative entries) * X >= 0, constant + (positive entries) * X < 2^31
bool row_fits(const int32_t* row, long long konst, long long x) {
    long long pos = 0, neg = 0;
    for (int i = 0; i < 3; ++i) { if (row[i] > 0) pos += row[i]; else neg += row[i]; }
    return konst + neg * x >= 0 && konst + pos * x < (1LL << 31);
}

bool vec_fits(const crtfx_egress* p, const void* src, size_t src_stride, const void* dst, size_t dst_stride, int n) {
    if (p->force_general || (p->args.w & 7)) return false;
    if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 3u) return false;
    return n <= 1 || !((src_stride | dst_stride) & 3u);
}

void note_plan(crtfx_egress* p, bool vec, int frames) {
    snprintf(p->plan, sizeof p->plan, "egress=k_egress_420<%s,%s>;frames=%d", p->layout == CRTFX_EGRESS_NV12 ? "nv12" : "yuv420p",
             vec ? "vec" : "general", frames);
}

}  // namespace

extern "C" {

const char* crtfx_egress_last_error(const crtfx_egress* p) { return p ? p->err.c_str() : g_create_err.c_str(); }

int crtfx_egress_create(int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, crtfx_egress** out_plan) {
    g_create_err.clear();
    if (!out_plan) return fail(nullptr, CRTFX_E_INVALID, "out_plan is null");
    *out_plan = nullptr;
    if (pix_fmt == CRTFX_PIX_F16) return fail(nullptr, CRTFX_E_UNSUPPORTED, "only uint8 RGB frames are converted (the egress stage takes finished frames)");
    if (pix_fmt != CRTFX_PIX_U8) return fail(nullptr, CRTFX_E_INVALID, "unknown pixel format %d", pix_fmt);
    if (h < 1 || w < 1 || h > 32767 || w > 32767) return fail(nullptr, CRTFX_E_INVALID, "size %dx%d outside 1..32767", h, w);
    if (layout != CRTFX_EGRESS_YUV420P && layout != CRTFX_EGRESS_NV12) return fail(nullptr, CRTFX_E_INVALID, "unknown layout %d", layout);
    if (!m || !off) return fail(nullptr, CRTFX_E_INVALID, "a table is null");
    for (int i = 0; i < 3; ++i)
        if (off[i] < 0 || off[i] > 255) return fail(nullptr, CRTFX_E_INVALID, "offset %d = %d outside 0..255", i, off[i]);
    const long long ky = ((long long)off[0] << SH) + (1LL << (SH - 1));
    const long long ku = ((long long)off[1] << (SH + 2)) + (1LL << (SH + 1)), kv = ((long long)off[2] << (SH + 2)) + (1LL << (SH + 1));
    if (!row_fits(m, ky, 255) || !row_fits(m + 3, ku, 1020) || !row_fits(m + 6, kv, 1020))
        return fail(nullptr, CRTFX_E_INVALID, "the matrix lets an accumulator leave [0, 2^31)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(nullptr, CRTFX_E_HIP, "no HIP device %d", device);
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return fail(nullptr, CRTFX_E_HIP, "hipSetDevice(%d): %s", device, hipGetErrorString(guard.err));
    crtfx_egress* p = new (std::nothrow) crtfx_egress();
    if (!p) return fail(nullptr, CRTFX_E_NOMEM, "out of host memory");
    p->device = device; p->layout = layout;
    Args& a = p->args;
    a.h = h; a.w = w; a.ch = (h + 1) / 2; a.cw = (w + 1) / 2;
    for (int i = 0; i < 9; ++i) a.m[i] = m[i];
    a.ky = (int)ky; a.ku = (int)ku; a.kv = (int)kv;
    p->frame_bytes = (size_t)h * w + 2 * (size_t)a.ch * a.cw;
    note_plan(p, vec_fits(p, nullptr, 0, nullptr, 0, 1), 0);
    *out_plan = p;
    return CRTFX_OK;
}

int crtfx_egress_destroy(crtfx_egress* p) {
    if (!p) return CRTFX_OK;
    DeviceGuard guard(p->device);
    (void)hipDeviceSynchronize();
    delete p;
    return CRTFX_OK;
}

size_t crtfx_egress_frame_bytes(const crtfx_egress* p) { return p ? p->frame_bytes : 0; }

int crtfx_egress_set_option(crtfx_egress* p, int option, int value) {
    if (!p) return CRTFX_E_INVALID;
    if (option != CRTFX_EGRESS_OPT_FORCE_GENERAL) return fail(p, CRTFX_E_INVALID, "unknown egress option %d", option);
    if (value != 0 && value != 1) return fail(p, CRTFX_E_INVALID, "FORCE_GENERAL takes 0 or 1, got %d", value);
    p->force_general = value != 0;
    note_plan(p, vec_fits(p, nullptr, 0, nullptr, 0, 1), 0);
    return CRTFX_OK;
}

int crtfx_egress_last_plan(crtfx_egress* p, char* buf, size_t n) {
    if (!p || !buf || n == 0) return CRTFX_E_INVALID;
    snprintf(buf, n, "%s", p->plan);
    return CRTFX_OK;
}

int crtfx_egress_run(crtfx_egress* p, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream) {
    if (!p) return CRTFX_E_INVALID;
    if (!src_base || !dst_base) return fail(p, CRTFX_E_INVALID, "null frame pointer");
    if (n < 1) return fail(p, CRTFX_E_INVALID, "n = %d frames", n);
    const size_t src_bytes = (size_t)p->args.h * p->args.w * 3;
    if (n > 1 && (src_stride_bytes < src_bytes || dst_stride_bytes < p->frame_bytes))
        return fail(p, CRTFX_E_INVALID, "frame strides %zu / %zu bytes are smaller than a frame (%zu / %zu)", src_stride_bytes, dst_stride_bytes, src_bytes, p->frame_bytes);
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return fail(p, CRTFX_E_HIP, "hipGetDevice failed");
    if (dev != p->device) return fail(p, CRTFX_E_INVALID, "current device %d is not the plan's device %d (call hipSetDevice first)", dev, p->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint8_t* src = static_cast<const uint8_t*>(src_base);
    uint8_t* dst = static_cast<uint8_t*>(dst_base);
    const bool vec = vec_fits(p, src_base, src_stride_bytes, dst_base, dst_stride_bytes, n);
    const bool nv12 = p->layout == CRTFX_EGRESS_NV12;
    const int items = vec ? p->args.ch * (p->args.w >> 3) : p->args.ch * p->args.cw;        // at most 16384 * 16384
    const int group = 32768;                                                                 // grid.z
    for (int f = 0; f < n; f += group) {
        Args a = p->args;
        a.src = src + (size_t)f * src_stride_bytes; a.src_stride = src_stride_bytes;
        a.dst = dst + (size_t)f * dst_stride_bytes; a.dst_stride = dst_stride_bytes;
        const dim3 grid((items + BLOCK - 1) / BLOCK, 1, n - f < group ? n - f : group);
        if (vec) {
            if (nv12) hipLaunchKernelGGL(k_egress_420_vec<true>, grid, dim3(BLOCK), 0, st, a);
            else hipLaunchKernelGGL(k_egress_420_vec<false>, grid, dim3(BLOCK), 0, st, a);
        } else {
            if (nv12) hipLaunchKernelGGL(k_egress_420_general<true>, grid, dim3(BLOCK), 0, st, a);
            else hipLaunchKernelGGL(k_egress_420_general<false>, grid, dim3(BLOCK), 0, st, a);
        }
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(p, CRTFX_E_HIP, "egress launch: %s", hipGetErrorString(e));
    }
    note_plan(p, vec, n);
    return CRTFX_OK;
}

}  // extern "C"
