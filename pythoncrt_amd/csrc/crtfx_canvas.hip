// crtfx_canvas.hip — the geometry stage (include/crtfx_canvas.h): one window of a frame moved to one place of a frame of another size, the
// rest filled with a colour.  Two kernels per sample type, the host glue, the C entry points.  No arithmetic: bytes are moved.

#include <hip/hip_runtime.h>

#include <cstdio>
#include <type_traits>

#include "crtfx_canvas.h"
#include "crtfx_frame_host.h"

namespace crtfx_canvas_impl {

struct u8 { using T = uint8_t; static constexpr const char* name = "u8"; };
struct f16 { using T = uint16_t; static constexpr const char* name = "f16"; };
struct vec {};
struct general {};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_dword_aligned __attribute__((aligned(4)));          // a 16-byte load at a dword-aligned address

// Launch constants.  Lengths and positions along a row are in UNITS: bytes for the vec kernel, samples for the general one.
struct Args {
    const uint8_t* src;
    uint8_t* dst;
    size_t src_stride, dst_stride;      // bytes
    uint32_t src_row, dst_row;          // units per row
    uint32_t src_len, dst_len;          // units per frame (vec: below 2^31; general: unused)
    uint32_t wx0, wx1;                  // the window's columns in the destination row: [wx0, wx1) units
    uint32_t sx;                        // the window's first column in the source row, units
    uint32_t win_y, win_h, dst_y;       // rows
    uint32_t pat0, pat1, pat2;          // vec: the fill colour's 12-byte pattern as the dwords at byte offsets 0, 4, 8 (mod 12) of a frame
    uint16_t fill[3];                   // general: per channel
    int wide;                           // vec: 16-byte stores (destination base and stride are multiples of 16)
};

constexpr int BLOCK = 256;

// (values first: a conditional over the members themselves is a conditional ADDRESS and a vector load from the argument segment)
__device__ __forceinline__ uint32_t pattern(const Args& a, uint32_t m) {
    const uint32_t p0 = a.pat0, p1 = a.pat1, p2 = a.pat2;
    return m == 0 ? p0 : m == 1 ? p1 : p2;
}

// the destination byte at frame offset o
__device__ __forceinline__ uint32_t byte_at(const uint8_t* __restrict__ s, const Args& a, uint32_t o) {
    const uint32_t y = o / a.dst_row, xb = o - y * a.dst_row, yy = y - a.dst_y;
    if (yy < a.win_h && xb >= a.wx0 && xb < a.wx1) return s[(a.win_y + yy) * a.src_row + a.sx + (xb - a.wx0)];
    return (pattern(a, (o >> 2) % 3u) >> (8u * (o & 3u))) & 0xffu;
}

// the destination dword at frame offset o (a multiple of 4) that lies in one row, at column xb of it.  row_in: the row is one of the
// placed window's; row: the source frame offset of that row's destination column 0 (mod 2^32: the window may start left of it)
__device__ __forceinline__ uint32_t dword_in_row(const uint8_t* __restrict__ s, const Args& a, uint32_t o, uint32_t xb, bool row_in, uint32_t row) {
    if (row_in && xb >= a.wx0 && xb + 4u <= a.wx1) {                   // four source bytes in a row, at frame offset so
        const uint32_t so = row + xb;
        const uint8_t* p = s + so;
        const uint32_t sh = (uint32_t)reinterpret_cast<uintptr_t>(p) & 3u;
        if (sh == 0) return *reinterpret_cast<const uint32_t*>(p);
        if (so >= sh && so - sh + 8u <= a.src_len) {                   // both aligned dwords lie inside the frame
            const uint32_t* q = reinterpret_cast<const uint32_t*>(p - sh);
            return __builtin_amdgcn_alignbit(q[1], q[0], 8u * sh);
        }
        return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    }
    const uint32_t f = pattern(a, (o >> 2) % 3u);
    if (!row_in || xb + 4u <= a.wx0 || xb >= a.wx1) return f;
    uint32_t v = 0;                                                    // a window edge inside the dword
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t xj = xb + j;
        const uint32_t b = xj >= a.wx0 && xj < a.wx1 ? (uint32_t)s[row + xj] : (f >> (8u * j)) & 0xffu;
        v |= b << (8u * j);
    }
    return v;
}

// the destination dword at frame offset o (a multiple of 4, o + 4 <= dst_len)
__device__ __forceinline__ uint32_t dword_at(const uint8_t* __restrict__ s, const Args& a, uint32_t o) {
    const uint32_t y = o / a.dst_row, xb = o - y * a.dst_row, yy = y - a.dst_y;
    if (xb + 4u <= a.dst_row) return dword_in_row(s, a, o, xb, yy < a.win_h, (a.win_y + yy) * a.src_row + a.sx - a.wx0);
    uint32_t v = 0;                                                    // a row end inside the dword
#pragma unroll 1
    for (uint32_t j = 0; j < 4; ++j) v |= byte_at(s, a, o + j) << (8u * j);
    return v;
}

// vec: one lane per aligned 16-byte chunk of the destination frame's bytes; units are bytes, so the sample type does not show
__device__ __forceinline__ void canvas_vec(const Args& a) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t o = i * 16u;
    if (o >= a.dst_len) return;
    const uint8_t* __restrict__ s = a.src + (size_t)blockIdx.z * a.src_stride;
    uint8_t* __restrict__ d = a.dst + (size_t)blockIdx.z * a.dst_stride + o;
    const bool whole = o + 16u <= a.dst_len;
    u32x4 v = {0, 0, 0, 0};
    bool done = false;
    if (whole) {
        const uint32_t y = o / a.dst_row, xb = o - y * a.dst_row, yy = y - a.dst_y;
        if (xb + 16u <= a.dst_row) {                                   // one row
            const bool row_in = yy < a.win_h;
            if (row_in && xb >= a.wx0 && xb + 16u <= a.wx1) {          // sixteen source bytes in a row, at frame offset so
                const uint32_t so = (a.win_y + yy) * a.src_row + a.sx + (xb - a.wx0);
                const uint8_t* p = s + so;
                const uint32_t sh = (uint32_t)reinterpret_cast<uintptr_t>(p) & 3u;
                if (so >= sh && so - sh + (sh ? 20u : 16u) <= a.src_len) {       // every aligned dword lies inside the frame
                    const uint32_t* q = reinterpret_cast<const uint32_t*>(p - sh);
                    const u32x4 w = *reinterpret_cast<const u32x4_dword_aligned*>(q);
                    if (sh) {
                        const uint32_t e = q[4], b = 8u * sh;
                        v.x = __builtin_amdgcn_alignbit(w.y, w.x, b);
                        v.y = __builtin_amdgcn_alignbit(w.z, w.y, b);
                        v.z = __builtin_amdgcn_alignbit(w.w, w.z, b);
                        v.w = __builtin_amdgcn_alignbit(e, w.w, b);
                    } else {
                        v = w;
                    }
                    done = true;
                }
            } else if (!row_in || xb + 16u <= a.wx0 || xb >= a.wx1) {  // a bar: the chunk starts at dword 4 i of the frame, 4 i = i (mod 3)
                const uint32_t m = i % 3u;
                v.x = pattern(a, m);
                v.y = pattern(a, m == 2 ? 0 : m + 1);
                v.z = pattern(a, m == 0 ? 2 : m - 1);
                v.w = v.x;
                done = true;
            }
            else {                                                     // a window edge inside the chunk: dword by dword, no division
                const uint32_t row = (a.win_y + yy) * a.src_row + a.sx - a.wx0;
                v.x = dword_in_row(s, a, o, xb, true, row);
                v.y = dword_in_row(s, a, o + 4u, xb + 4u, true, row);
                v.z = dword_in_row(s, a, o + 8u, xb + 8u, true, row);
                v.w = dword_in_row(s, a, o + 12u, xb + 12u, true, row);
                done = true;
            }
        }
    }
    if (!done) {                                                       // a row end, a frame end, the first or last dword of the source frame: dword by dword
#pragma unroll 1
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t r = o + 4u * k < a.dst_len ? dword_at(s, a, o + 4u * k) : 0u;
            v.x = k == 0 ? r : v.x; v.y = k == 1 ? r : v.y; v.z = k == 2 ? r : v.z; v.w = k == 3 ? r : v.w;
        }
    }
    if (whole && a.wide) {
        *reinterpret_cast<u32x4*>(d) = v;
    } else {
        uint32_t* dd = reinterpret_cast<uint32_t*>(d);
        dd[0] = v.x;
        if (o + 4u < a.dst_len) dd[1] = v.y;
        if (o + 8u < a.dst_len) dd[2] = v.z;
        if (o + 12u < a.dst_len) dd[3] = v.w;
    }
}

// general: one lane per destination sample; units are samples
template <class S>
__device__ __forceinline__ void canvas_general(const Args& a) {
    using T = typename S::T;
    const uint32_t xs = blockIdx.x * BLOCK + threadIdx.x, y = blockIdx.y;
    if (xs >= a.dst_row) return;
    const T* __restrict__ s = reinterpret_cast<const T*>(a.src + (size_t)blockIdx.z * a.src_stride);
    T* __restrict__ d = reinterpret_cast<T*>(a.dst + (size_t)blockIdx.z * a.dst_stride);
    const uint32_t yy = y - a.dst_y;
    T v;
    if (yy < a.win_h && xs >= a.wx0 && xs < a.wx1) {
        v = s[(size_t)(a.win_y + yy) * a.src_row + a.sx + (xs - a.wx0)];
    } else {
        const uint32_t c = xs % 3u;
        const T f0 = (T)a.fill[0], f1 = (T)a.fill[1], f2 = (T)a.fill[2];
        v = c == 0 ? f0 : c == 1 ? f1 : f2;
    }
    d[(size_t)y * a.dst_row + xs] = v;
}

template <class S, class Path>
__global__ __launch_bounds__(BLOCK) void k_canvas(Args a) {
    if constexpr (std::is_same<Path, vec>::value) canvas_vec(a); else canvas_general<S>(a);
}

}  // namespace crtfx_canvas_impl

using namespace crtfx_canvas_impl;

struct crtfx_canvas : crtfx_frames::Plan {     // src_bps == dst_bps
    int src_h = 0, src_w = 0, win_y = 0, win_x = 0, win_h = 0, win_w = 0, dst_h = 0, dst_w = 0, dst_y = 0, dst_x = 0;
    uint16_t fill[3] = {0, 0, 0};
};

namespace {

using crtfx_frames::Batch;
using crtfx_stage::create_err;
using crtfx_stage::fail;

struct U : crtfx_frames::Unit {
    using H = crtfx_canvas;
    static constexpr int force_option = CRTFX_CANVAS_OPT_FORCE_GENERAL;
    static constexpr const char* name = "canvas";

    // the vec kernel's conditions (crtfx_canvas.h)
    static bool vec_fits(const H* p, const Batch& b) {
        if (p->force_general || (p->dst_bytes & 3u) || p->dst_bytes >= (1ull << 31) || p->src_bytes >= (1ull << 31)) return false;
        if (reinterpret_cast<uintptr_t>(b.dst) & 3u) return false;
        return b.n <= 1 || !(b.dst_stride & 3u);
    }

    static void note_plan(H* p, bool vec, int frames) {
        snprintf(p->plan, sizeof p->plan, "canvas=k_canvas<%s,%s>;frames=%d", p->src_bps == 2 ? f16::name : u8::name, vec ? "vec" : "general", frames);
    }

    static Args make_args(const H* p, bool vec, const Batch& b) {
        Args a{};
        const uint32_t unit = vec ? 3u * p->src_bps : 3u;               // units per pixel
        a.src_row = p->src_w * unit; a.dst_row = p->dst_w * unit;
        a.src_len = vec ? (uint32_t)p->src_bytes : 0; a.dst_len = vec ? (uint32_t)p->dst_bytes : 0;
        a.wx0 = p->dst_x * unit; a.wx1 = (p->dst_x + p->win_w) * unit; a.sx = p->win_x * unit;
        a.win_y = p->win_y; a.win_h = p->win_h; a.dst_y = p->dst_y;
        uint8_t bytes[12];                                              // two pixels of half, four of uint8: twelve bytes either way
        for (int i = 0; i < 12; ++i)
            bytes[i] = p->src_bps == 2 ? (uint8_t)(p->fill[(i / 2) % 3] >> (8 * (i & 1))) : (uint8_t)p->fill[i % 3];
        a.pat0 = bytes[0] | bytes[1] << 8 | bytes[2] << 16 | (uint32_t)bytes[3] << 24;
        a.pat1 = bytes[4] | bytes[5] << 8 | bytes[6] << 16 | (uint32_t)bytes[7] << 24;
        a.pat2 = bytes[8] | bytes[9] << 8 | bytes[10] << 16 | (uint32_t)bytes[11] << 24;
        for (int c = 0; c < 3; ++c) a.fill[c] = p->fill[c];
        a.wide = !(reinterpret_cast<uintptr_t>(b.dst) & 15u) && (b.n <= 1 || !(b.dst_stride & 15u));
        return a;
    }

    static void launch(const H* p, bool fits, Args& a, int, unsigned g, hipStream_t st) {
        if (fits) {
            const dim3 grid((unsigned)((p->dst_bytes + 16u * BLOCK - 1) / (16u * BLOCK)), 1, g);
            if (p->src_bps == 2) hipLaunchKernelGGL((k_canvas<f16, vec>), grid, dim3(BLOCK), 0, st, a);
            else hipLaunchKernelGGL((k_canvas<u8, vec>), grid, dim3(BLOCK), 0, st, a);
        } else {
            const dim3 grid((a.dst_row + BLOCK - 1) / BLOCK, p->dst_h, g);
            if (p->src_bps == 2) hipLaunchKernelGGL((k_canvas<f16, general>), grid, dim3(BLOCK), 0, st, a);
            else hipLaunchKernelGGL((k_canvas<u8, general>), grid, dim3(BLOCK), 0, st, a);
        }
    }
};

}  // namespace

extern "C" {

const char* crtfx_canvas_last_error(const crtfx_canvas* p) { return p ? p->err.c_str() : create_err<crtfx_canvas>().c_str(); }

int crtfx_canvas_create(int device, int pix_fmt, int src_h, int src_w, int win_y, int win_x, int win_h, int win_w,
                        int dst_h, int dst_w, int dst_y, int dst_x, const uint16_t fill[3], crtfx_canvas** out_plan) {
    using H = crtfx_canvas;
    if (const int rc = crtfx_frames::begin_create(out_plan)) return rc;
    if (pix_fmt != CRTFX_PIX_U8 && pix_fmt != CRTFX_PIX_F16) return fail<H>(nullptr, CRTFX_E_INVALID, "unknown pixel format %d", pix_fmt);
    if (!fill) return fail<H>(nullptr, CRTFX_E_INVALID, "fill is null");
    const struct { const char* name; int v; } sizes[] = {{"src_h", src_h}, {"src_w", src_w}, {"win_h", win_h}, {"win_w", win_w}, {"dst_h", dst_h}, {"dst_w", dst_w}};
    for (const auto& s : sizes)
        if (const int rc = crtfx_frames::check_size<H>(s.name, s.v)) return rc;
    if (win_y < 0 || win_y > src_h - win_h)
        return fail<H>(nullptr, CRTFX_E_INVALID, "win_y = %d: the window's rows %d..%d leave the source's %d", win_y, win_y, win_y + win_h, src_h);
    if (win_x < 0 || win_x > src_w - win_w)
        return fail<H>(nullptr, CRTFX_E_INVALID, "win_x = %d: the window's columns %d..%d leave the source's %d", win_x, win_x, win_x + win_w, src_w);
    if (dst_y < 0 || dst_y > dst_h - win_h)
        return fail<H>(nullptr, CRTFX_E_INVALID, "dst_y = %d: the placed rows %d..%d leave the destination's %d", dst_y, dst_y, dst_y + win_h, dst_h);
    if (dst_x < 0 || dst_x > dst_w - win_w)
        return fail<H>(nullptr, CRTFX_E_INVALID, "dst_x = %d: the placed columns %d..%d leave the destination's %d", dst_x, dst_x, dst_x + win_w, dst_w);
    if (pix_fmt == CRTFX_PIX_U8)
        for (int c = 0; c < 3; ++c)
            if (fill[c] > 255) return fail<H>(nullptr, CRTFX_E_INVALID, "fill[%d] = %d outside 0..255 for uint8 frames", c, (int)fill[c]);
    return crtfx_frames::new_plan<U>(device, out_plan, [&](H* p) {
        p->src_bps = p->dst_bps = pix_fmt == CRTFX_PIX_F16 ? 2 : 1;
        p->src_h = src_h; p->src_w = src_w; p->win_y = win_y; p->win_x = win_x; p->win_h = win_h; p->win_w = win_w;
        p->dst_h = dst_h; p->dst_w = dst_w; p->dst_y = dst_y; p->dst_x = dst_x;
        for (int c = 0; c < 3; ++c) p->fill[c] = fill[c];
        p->src_bytes = (size_t)src_h * src_w * 3 * p->src_bps;
        p->dst_bytes = (size_t)dst_h * dst_w * 3 * p->dst_bps;
        return CRTFX_OK;
    });
}

int crtfx_canvas_destroy(crtfx_canvas* p) { return crtfx_frames::destroy(p); }

int crtfx_canvas_set_option(crtfx_canvas* p, int option, int value) { return crtfx_frames::set_option<U>(p, option, value); }

int crtfx_canvas_last_plan(crtfx_canvas* p, char* buf, size_t n) { return crtfx_frames::last_plan(p, buf, n); }

int crtfx_canvas_run(crtfx_canvas* p, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream) {
    return crtfx_frames::run<U>(p, Batch{nullptr, src_base, src_stride_bytes, dst_base, dst_stride_bytes, n}, stream);
}

}  // extern "C"

