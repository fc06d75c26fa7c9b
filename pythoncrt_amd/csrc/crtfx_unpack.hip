// crtfx_unpack.hip — the source stage of libcrtfx.so (include/crtfx_unpack.h): uint8 yuv420p / nv12 frames -> uint8 RGB on the device.
// A translation unit of its own: it shares no kernel, table or handle with the effect chain, the ingest stage or the egress stage.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>

#include "crtfx_unpack.h"

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

struct crtfx_unpack {
    int device = 0;
    int layout = CRTFX_UNPACK_YUV420P;
    Args args{};                        // launch constants (frame pointers filled per run)
    size_t frame_bytes = 0;
    bool force_general = false;
    char plan[128] = "";
    std::string err;
};

namespace {

thread_local std::string g_create_err;

int fail(crtfx_unpack* p, int code, const char* fmt, ...) {
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

// the accumulator of one row stays inside int32 for every input: |c|, |d|, |e| <= 255
bool row_fits(const int32_t* row) {
    long long s = 1LL << (SH - 1);
    for (int i = 0; i < 3; ++i) s += (row[i] < 0 ? -(long long)row[i] : (long long)row[i]) * 255;
    return s < (1LL << 31);
}

bool vec_fits(const crtfx_unpack* p, const void* src, size_t src_stride, const void* dst, size_t dst_stride, int n) {
    if (p->force_general || (p->args.w & 7)) return false;
    if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 3u) return false;
    return n <= 1 || !((src_stride | dst_stride) & 3u);
}

void note_plan(crtfx_unpack* p, bool vec, int frames) {
    snprintf(p->plan, sizeof p->plan, "unpack=k_unpack_420<%s,%s>;frames=%d", p->layout == CRTFX_UNPACK_NV12 ? "nv12" : "yuv420p",
             vec ? "vec" : "general", frames);
}

}  // namespace

extern "C" {

const char* crtfx_unpack_last_error(const crtfx_unpack* p) { return p ? p->err.c_str() : g_create_err.c_str(); }

int crtfx_unpack_create(int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, crtfx_unpack** out_plan) {
    g_create_err.clear();
    if (!out_plan) return fail(nullptr, CRTFX_E_INVALID, "out_plan is null");
    *out_plan = nullptr;
    if (pix_fmt == CRTFX_PIX_F16) return fail(nullptr, CRTFX_E_UNSUPPORTED, "only uint8 RGB frames are written (the source stage feeds the chain's uint8 input)");
    if (pix_fmt != CRTFX_PIX_U8) return fail(nullptr, CRTFX_E_INVALID, "unknown pixel format %d", pix_fmt);
    if (h < 1 || w < 1 || h > 32767 || w > 32767) return fail(nullptr, CRTFX_E_INVALID, "size %dx%d outside 1..32767", h, w);
    if (layout != CRTFX_UNPACK_YUV420P && layout != CRTFX_UNPACK_NV12) return fail(nullptr, CRTFX_E_INVALID, "unknown layout %d", layout);
    if (!m || !off) return fail(nullptr, CRTFX_E_INVALID, "a table is null");
    for (int i = 0; i < 3; ++i)
        if (off[i] < 0 || off[i] > 255) return fail(nullptr, CRTFX_E_INVALID, "offset %d = %d outside 0..255", i, off[i]);
    if (!row_fits(m) || !row_fits(m + 3) || !row_fits(m + 6))
        return fail(nullptr, CRTFX_E_INVALID, "the matrix lets an accumulator leave int32");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(nullptr, CRTFX_E_HIP, "no HIP device %d", device);
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return fail(nullptr, CRTFX_E_HIP, "hipSetDevice(%d): %s", device, hipGetErrorString(guard.err));
    crtfx_unpack* p = new (std::nothrow) crtfx_unpack();
    if (!p) return fail(nullptr, CRTFX_E_NOMEM, "out of host memory");
    p->device = device; p->layout = layout;
    Args& a = p->args;
    a.h = h; a.w = w; a.ch = (h + 1) / 2; a.cw = (w + 1) / 2;
    for (int i = 0; i < 9; ++i) a.m[i] = m[i];
    for (int i = 0; i < 3; ++i) a.off[i] = off[i];
    p->frame_bytes = (size_t)h * w + 2 * (size_t)a.ch * a.cw;
    note_plan(p, vec_fits(p, nullptr, 0, nullptr, 0, 1), 0);
    *out_plan = p;
    return CRTFX_OK;
}

int crtfx_unpack_destroy(crtfx_unpack* p) {
    if (!p) return CRTFX_OK;
    DeviceGuard guard(p->device);
    (void)hipDeviceSynchronize();
    delete p;
    return CRTFX_OK;
}

size_t crtfx_unpack_frame_bytes(const crtfx_unpack* p) { return p ? p->frame_bytes : 0; }

int crtfx_unpack_set_option(crtfx_unpack* p, int option, int value) {
    if (!p) return CRTFX_E_INVALID;
    if (option != CRTFX_UNPACK_OPT_FORCE_GENERAL) return fail(p, CRTFX_E_INVALID, "unknown unpack option %d", option);
    if (value != 0 && value != 1) return fail(p, CRTFX_E_INVALID, "FORCE_GENERAL takes 0 or 1, got %d", value);
    p->force_general = value != 0;
    note_plan(p, vec_fits(p, nullptr, 0, nullptr, 0, 1), 0);
    return CRTFX_OK;
}

int crtfx_unpack_last_plan(crtfx_unpack* p, char* buf, size_t n) {
    if (!p || !buf || n == 0) return CRTFX_E_INVALID;
    snprintf(buf, n, "%s", p->plan);
    return CRTFX_OK;
}

int crtfx_unpack_run(crtfx_unpack* p, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream) {
    if (!p) return CRTFX_E_INVALID;
    if (!src_base || !dst_base) return fail(p, CRTFX_E_INVALID, "null frame pointer");
    if (n < 1) return fail(p, CRTFX_E_INVALID, "n = %d frames", n);
    const size_t dst_bytes = (size_t)p->args.h * p->args.w * 3;
    if (n > 1 && (src_stride_bytes < p->frame_bytes || dst_stride_bytes < dst_bytes))
        return fail(p, CRTFX_E_INVALID, "frame strides %zu / %zu bytes are smaller than a frame (%zu / %zu)", src_stride_bytes, dst_stride_bytes, p->frame_bytes, dst_bytes);
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return fail(p, CRTFX_E_HIP, "hipGetDevice failed");
    if (dev != p->device) return fail(p, CRTFX_E_INVALID, "current device %d is not the plan's device %d (call hipSetDevice first)", dev, p->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint8_t* src = static_cast<const uint8_t*>(src_base);
    uint8_t* dst = static_cast<uint8_t*>(dst_base);
    const bool vec = vec_fits(p, src_base, src_stride_bytes, dst_base, dst_stride_bytes, n);
    const bool nv12 = p->layout == CRTFX_UNPACK_NV12;
    const int items = vec ? p->args.ch * (p->args.w >> 3) : p->args.ch * p->args.cw;        // at most 16384 * 16384
    const int group = 32768;                                                                 // grid.z
    for (int f = 0; f < n; f += group) {
        Args a = p->args;
        a.src = src + (size_t)f * src_stride_bytes; a.src_stride = src_stride_bytes;
        a.dst = dst + (size_t)f * dst_stride_bytes; a.dst_stride = dst_stride_bytes;
        const dim3 grid((items + BLOCK - 1) / BLOCK, 1, n - f < group ? n - f : group);
        if (vec) {
            if (nv12) hipLaunchKernelGGL(k_unpack_420_vec<true>, grid, dim3(BLOCK), 0, st, a);
            else hipLaunchKernelGGL(k_unpack_420_vec<false>, grid, dim3(BLOCK), 0, st, a);
        } else {
            if (nv12) hipLaunchKernelGGL(k_unpack_420_general<true>, grid, dim3(BLOCK), 0, st, a);
            else hipLaunchKernelGGL(k_unpack_420_general<false>, grid, dim3(BLOCK), 0, st, a);
        }
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(p, CRTFX_E_HIP, "unpack launch: %s", hipGetErrorString(e));
    }
    note_plan(p, vec, n);
    return CRTFX_OK;
}

}  // extern "C"
