// crtfx_egress_field420.hip — the field-paired 4:2:0 egress stage of libcrtfx.so (include/crtfx_egress_field420.h): finished RGB frames ->
// yuv420p / nv12 / yuv420p10le / p010le with every chroma sample formed from luma rows of its own field only.  A translation unit of its
// own: it shares no kernel, table or handle with the effect chain or the other stages; the loaders, the quantiser and the stores are those
// of crtfx_egress_sited.hip's 4:2:0 layouts, restated here because that unit's builds are held to their register counts.  The host code
// around the kernels (checks, frame-group loop, error strings) is the skeleton of crtfx_stage_host.h; the chroma option is this unit's own.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <type_traits>

#include "crtfx_egress_field420.h"
#include "crtfx_stage_host.h"

namespace crtfx_egress_field420_impl {

constexpr int BLOCK = 256;
constexpr int SH = 16;                          // fractional bits of the matrix
constexpr int CSH = SH + 6;                     // the shift of a chroma sum: horizontal weights sum to 4, vertical ones to 16
constexpr int GENERAL = 0, VEC = 1;             // the PATH template argument; LAYOUT is a crtfx_field420_layout

struct Args {
    const uint8_t* src; size_t src_stride;
    uint8_t* dst; size_t dst_stride;
    int h, w, ch, cw;                           // ch = h / 2 chroma rows, which are also the luma rows of one field
    int m[9];                                   // rows Y, U, V over the columns R, G, B
    unsigned k[3];                              // (off0 << SH) + half for Y; (off << CSH) + half for U, V (10-bit: up to 2^31 + 2^21)
    int wt[3];                                  // the horizontal weights of the pixel left of, on and right of column 2 cx, in quarters
    int vt[4], vb[4];                           // the vertical weights of field rows 2 i - 1 .. 2 i + 2, in sixteenths: top field, bottom field
};

// unsigned dwords at 4-byte alignment: the widest access the vec path's rule (crtfx_egress_field420.h) guarantees
struct __attribute__((packed, aligned(4))) U2 { unsigned v[2]; };
struct __attribute__((packed, aligned(4))) U4 { unsigned v[4]; };
struct __attribute__((packed, aligned(4))) U6 { unsigned v[6]; };
struct __attribute__((packed, aligned(4))) U12 { unsigned v[12]; };

template <int LAYOUT> struct Traits {
    static constexpr bool deep = LAYOUT == CRTFX_FIELD420_YUV420P10LE || LAYOUT == CRTFX_FIELD420_P010LE;
    static constexpr bool p010 = LAYOUT == CRTFX_FIELD420_P010LE;
    static constexpr bool semi = LAYOUT == CRTFX_FIELD420_NV12 || p010;                                    // one plane of (U, V) pairs
    static constexpr unsigned top = deep ? 1023u : 255u;       // the largest sample
    using Row = typename std::conditional<deep, U12, U6>::type;                                            // 8 RGB pixels of one row
};

// the quarter code of a half bit pattern, exactly crtfx_deep.hip's: rint_to_even(min(max(4 f, 0), 1020)), NaN -> 0.  The half -> float
// conversion and 4 f are exact; a NaN fails `> 0` and takes the 0, as -0, negatives and -inf do; +inf takes 1020.
__device__ __forceinline__ int quantise(unsigned bits16) {
    float t = 4.0f * (float)__builtin_bit_cast(_Float16, (unsigned short)bits16);
    t = t > 0.0f ? t : 0.0f;
    t = t < 1020.0f ? t : 1020.0f;
    return (int)rintf(t);
}

// create admits only matrices whose accumulators stay in [0, 2^32) — the 10-bit chroma ones pass 2^31 — so every sum is formed in
// UNSIGNED 32-bit arithmetic: congruent to the integer sum modulo 2^32 whatever the intermediate terms do, hence equal to it (the header
// has the proof).  The lower clamp can never act, the shift is a logical one and the upper clamp is an unsigned minimum.
template <int LAYOUT> __device__ __forceinline__ unsigned luma(const Args& a, const int (&p)[3]) {
    return min(((unsigned)a.m[0] * (unsigned)p[0] + (unsigned)a.m[1] * (unsigned)p[1] + (unsigned)a.m[2] * (unsigned)p[2] + a.k[0]) >> SH, Traits<LAYOUT>::top);
}
template <int LAYOUT> __device__ __forceinline__ unsigned chroma(const Args& a, int row, const int (&s)[3]) {
    return min(((unsigned)a.m[3 * row] * (unsigned)s[0] + (unsigned)a.m[3 * row + 1] * (unsigned)s[1] + (unsigned)a.m[3 * row + 2] * (unsigned)s[2] + a.k[row]) >> CSH,
               Traits<LAYOUT>::top);
}
// the 16-bit word of a 10-bit sample: bits outside the sample are written 0
template <int LAYOUT> __device__ __forceinline__ unsigned word(unsigned v) { return Traits<LAYOUT>::p010 ? v << 6 : v; }

// the per-pixel codes of pixel (y, x) with narrow loads: 3 bytes, or 3 halves through the quantiser
template <int LAYOUT>
__device__ __forceinline__ void pixel_at(const uint8_t* fsrc, const Args& a, int y, int x, int (&p)[3]) {
    const size_t o = ((size_t)y * a.w + x) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = Traits<LAYOUT>::deep ? quantise(reinterpret_cast<const uint16_t*>(fsrc)[o + c]) : (int)fsrc[o + c];
}

// pixel i (0..7) of a lane's row block
template <int LAYOUT>
__device__ __forceinline__ void pixel_of(const typename Traits<LAYOUT>::Row& r, int i, int (&p)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int b = 3 * i + c;
        if (Traits<LAYOUT>::deep) p[c] = quantise((b & 1) ? r.v[b >> 1] >> 16 : r.v[b >> 1] & 0xFFFFu);
        else p[c] = (int)((r.v[b >> 2] >> (8 * (b & 3))) & 255u);
    }
}

// Lane rows are the ch chroma rows: lane row c serves field f = c & 1 and that field's chroma row i = c >> 1, that is the luma rows
// 4 i + f and 4 i + 2 + f (h % 4 == 0: both always inside the frame), so consecutive lane rows touch consecutive frame rows.  The four
// vertical taps are the field rows 2 i - 1 .. 2 i + 2 clamped to [0, ch - 1]; taps 1 and 2 are the lane's own two rows, whose Y it stores.
// vec (w % 8 == 0, 4-byte-aligned frame bases): one lane = 8 columns; consecutive lanes, consecutive column blocks.  One row of RGB is
//     in hand at a time: its H goes into the twelve running sums (four chroma samples x three channels) with the row's weight.  The
//     pixel left of the block is read with one narrow load per row at a clamped index.
// general: one lane = one chroma sample and the (up to) 2 x 2 luma samples of its field under it; bytes (8-bit) or 16-bit words (10-bit).
template <int LAYOUT, int PATH>
__global__ __launch_bounds__(BLOCK) void k_egress_field420(Args a) {
    using T = Traits<LAYOUT>;
    const uint8_t* fsrc = a.src + (size_t)blockIdx.z * a.src_stride;
    uint8_t* fdst = a.dst + (size_t)blockIdx.z * a.dst_stride;
    const int idx = blockIdx.x * BLOCK + threadIdx.x;
    const int per_row = PATH == VEC ? a.w >> 3 : a.cw;
    if (idx >= a.ch * per_row) return;
    const int c = idx / per_row, bx = idx - c * per_row;       // general: bx is the chroma column
    const int f = c & 1, i = c >> 1;
    int yy[4], vw[4];                                          // the frame rows of the four taps and their weights
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        yy[t] = 2 * min(max(2 * i - 1 + t, 0), a.ch - 1) + f;
        vw[t] = f ? a.vb[t] : a.vt[t];
    }
    const size_t E = T::deep ? 2 : 1;                          // bytes of a sample
    if (PATH == VEC) {
        int s[4][3] = {};                                      // S of the lane's four chroma samples
        const int xl = max(8 * bx - 1, 0);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const typename T::Row blk = *reinterpret_cast<const typename T::Row*>(fsrc + ((size_t)yy[t] * a.w + (size_t)bx * 8) * 3 * E);
            int prev[3];                                       // the pixel left of the one in hand; first the one left of the block
            pixel_at<LAYOUT>(fsrc, a, yy[t], xl, prev);
            unsigned yq[8];
#pragma unroll
            for (int q = 0; q < 4; ++q) {                      // chroma sample q = columns 2q (where "left" sits), 2q + 1
                int own[3], right[3];
                pixel_of<LAYOUT>(blk, 2 * q, own);
                pixel_of<LAYOUT>(blk, 2 * q + 1, right);
                if (t == 1 || t == 2) { yq[2 * q] = luma<LAYOUT>(a, own); yq[2 * q + 1] = luma<LAYOUT>(a, right); }
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    s[q][ch] += vw[t] * (a.wt[0] * prev[ch] + a.wt[1] * own[ch] + a.wt[2] * right[ch]);
                    prev[ch] = right[ch];
                }
            }
            if (t == 1 || t == 2) {                            // the lane's own rows: 4 i + f and 4 i + 2 + f, never clamped
                if (T::deep) {
                    U4 o;
#pragma unroll
                    for (int j = 0; j < 4; ++j) o.v[j] = word<LAYOUT>(yq[2 * j]) | (word<LAYOUT>(yq[2 * j + 1]) << 16);
                    *reinterpret_cast<U4*>(fdst + ((size_t)yy[t] * a.w + (size_t)bx * 8) * 2) = o;
                } else {
                    U2 o;
#pragma unroll
                    for (int j = 0; j < 2; ++j) o.v[j] = yq[4 * j] | (yq[4 * j + 1] << 8) | (yq[4 * j + 2] << 16) | (yq[4 * j + 3] << 24);
                    *reinterpret_cast<U2*>(fdst + (size_t)yy[t] * a.w + (size_t)bx * 8) = o;
                }
            }
        }
        unsigned uq[4], vq[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { uq[q] = chroma<LAYOUT>(a, 1, s[q]); vq[q] = chroma<LAYOUT>(a, 2, s[q]); }
        // ---- chroma stores: the dword-multiple accesses of the layout's sited kernel, chroma row c ----
        uint8_t* cbase = fdst + (size_t)a.h * a.w * E;
        const size_t plane = (size_t)a.ch * a.cw * E;
        if (T::deep && T::semi) {               // u0 v0 | u1 v1 | u2 v2 | u3 v3
            U4 uv;
#pragma unroll
            for (int q = 0; q < 4; ++q) uv.v[q] = word<LAYOUT>(uq[q]) | (word<LAYOUT>(vq[q]) << 16);
            *reinterpret_cast<U4*>(cbase + (size_t)c * a.w * 2 + (size_t)bx * 16) = uv;
        } else if (T::deep) {
            const size_t o = ((size_t)c * a.cw + (size_t)bx * 4) * 2;
            U2 up, vp;
#pragma unroll
            for (int j = 0; j < 2; ++j) { up.v[j] = word<LAYOUT>(uq[2 * j]) | (word<LAYOUT>(uq[2 * j + 1]) << 16); vp.v[j] = word<LAYOUT>(vq[2 * j]) | (word<LAYOUT>(vq[2 * j + 1]) << 16); }
            *reinterpret_cast<U2*>(cbase + o) = up;
            *reinterpret_cast<U2*>(cbase + plane + o) = vp;
        } else if (T::semi) {                   // u0 v0 u1 v1 | u2 v2 u3 v3
            U2 uv;
#pragma unroll
            for (int j = 0; j < 2; ++j) uv.v[j] = uq[2 * j] | (vq[2 * j] << 8) | (uq[2 * j + 1] << 16) | (vq[2 * j + 1] << 24);
            *reinterpret_cast<U2*>(cbase + (size_t)c * a.w + (size_t)bx * 8) = uv;
        } else {
            const size_t o = (size_t)c * a.cw + (size_t)bx * 4;
            *reinterpret_cast<unsigned*>(cbase + o) = uq[0] | (uq[1] << 8) | (uq[2] << 16) | (uq[3] << 24);
            *reinterpret_cast<unsigned*>(cbase + plane + o) = vq[0] | (vq[1] << 8) | (vq[2] << 16) | (vq[3] << 24);
        }
    } else {
        const int x0 = 2 * bx;
        const bool right = x0 + 1 < a.w;
        const int xl = max(x0 - 1, 0), xr = right ? x0 + 1 : x0;
        int s[3] = {0, 0, 0};
        unsigned ya[2], yb[2];                  // the Y of columns x0 and xr in the lane's own two rows
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            int pl[3], p0[3], pr[3];
            pixel_at<LAYOUT>(fsrc, a, yy[t], xl, pl);
            pixel_at<LAYOUT>(fsrc, a, yy[t], x0, p0);
            pixel_at<LAYOUT>(fsrc, a, yy[t], xr, pr);
            if (t == 1 || t == 2) { ya[t - 1] = luma<LAYOUT>(a, p0); yb[t - 1] = luma<LAYOUT>(a, pr); }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) s[ch] += vw[t] * (a.wt[0] * pl[ch] + a.wt[1] * p0[ch] + a.wt[2] * pr[ch]);
        }
        const unsigned u = chroma<LAYOUT>(a, 1, s), v = chroma<LAYOUT>(a, 2, s);
        const size_t o = (size_t)c * a.cw + bx, plane = (size_t)a.ch * a.cw, luma_n = (size_t)a.h * a.w;
        if (T::deep) {
            uint16_t* f16 = reinterpret_cast<uint16_t*>(fdst);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                uint16_t* y = f16 + (size_t)yy[r + 1] * a.w + x0;
                y[0] = (uint16_t)word<LAYOUT>(ya[r]);
                if (right) y[1] = (uint16_t)word<LAYOUT>(yb[r]);
            }
            uint16_t* cb = f16 + luma_n;
            if (T::semi) { cb[2 * o] = (uint16_t)word<LAYOUT>(u); cb[2 * o + 1] = (uint16_t)word<LAYOUT>(v); }
            else { cb[o] = (uint16_t)word<LAYOUT>(u); cb[plane + o] = (uint16_t)word<LAYOUT>(v); }
        } else {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                uint8_t* y = fdst + (size_t)yy[r + 1] * a.w + x0;
                y[0] = (uint8_t)ya[r];
                if (right) y[1] = (uint8_t)yb[r];
            }
            uint8_t* cb = fdst + luma_n;
            if (T::semi) { cb[2 * o] = (uint8_t)u; cb[2 * o + 1] = (uint8_t)v; }
            else { cb[o] = (uint8_t)u; cb[plane + o] = (uint8_t)v; }
        }
    }
}

}  // namespace crtfx_egress_field420_impl

using namespace crtfx_egress_field420_impl;
using namespace crtfx_stage;

struct crtfx_egress_field420 : StagePlan { Args args{}; int chroma = CRTFX_EGRESS_FIELD420_CENTER; };        // `egress` is always true

namespace {

static_assert(SH == MATRIX_SH, "the matrices are the other egress stages'");

const char* const LAYOUT_NAMES[4] = {"yuv420p", "nv12", "yuv420p10le", "p010le"};
bool is_deep(int layout) { return layout == CRTFX_FIELD420_YUV420P10LE || layout == CRTFX_FIELD420_P010LE; }

template <int LAYOUT>
void launch_layout(bool vec, dim3 grid, hipStream_t st, const Args& a) {
    if (vec) hipLaunchKernelGGL((k_egress_field420<LAYOUT, VEC>), grid, dim3(BLOCK), 0, st, a);
    else hipLaunchKernelGGL((k_egress_field420<LAYOUT, GENERAL>), grid, dim3(BLOCK), 0, st, a);
}

struct Unit {
    static constexpr int block = BLOCK, force_option = CRTFX_EGRESS_FIELD420_OPT_FORCE_GENERAL;
    static const char* name(bool) { return "egress_field420"; }
    static void note_plan(crtfx_egress_field420* p, bool vec, int frames) {
        snprintf(p->plan, sizeof p->plan, "egress_field420=k_egress_field420<%s,%s>;chroma=%s;frames=%d", LAYOUT_NAMES[p->layout], vec ? "vec" : "general",
                 p->chroma == CRTFX_EGRESS_FIELD420_LEFT ? "left" : "center", frames);
    }
    static int check_alignment(crtfx_egress_field420* p, const void* src_base, size_t src_stride_bytes, const void* dst_base, size_t dst_stride_bytes) {
        if (is_deep(p->layout) && ((reinterpret_cast<uintptr_t>(src_base) | reinterpret_cast<uintptr_t>(dst_base) | src_stride_bytes | dst_stride_bytes) & 1u))
            return fail(p, CRTFX_E_INVALID, "an odd frame base or stride: 16-bit samples need 2-byte alignment");
        return CRTFX_OK;                                                                                  // bytes: any base, any stride
    }
    static int items(const Args& a, bool vec) { return a.ch * (vec ? a.w >> 3 : a.cw); }                 // at most 16383 * 16384
    static void launch(const crtfx_egress_field420* p, bool vec, dim3 grid, hipStream_t st, const Args& a) {
        switch (p->layout) {
            case CRTFX_FIELD420_NV12: launch_layout<CRTFX_FIELD420_NV12>(vec, grid, st, a); break;
            case CRTFX_FIELD420_YUV420P10LE: launch_layout<CRTFX_FIELD420_YUV420P10LE>(vec, grid, st, a); break;
            case CRTFX_FIELD420_P010LE: launch_layout<CRTFX_FIELD420_P010LE>(vec, grid, st, a); break;
            default: launch_layout<CRTFX_FIELD420_YUV420P>(vec, grid, st, a); break;
        }
    }
};

// the weights of crtfx_egress_field420.h: horizontal in quarters, vertical in sixteenths over field rows 2 i - 1 .. 2 i + 2
void set_chroma(crtfx_egress_field420* p, int chroma) {
    Args& a = p->args;
    p->chroma = chroma;
    const bool left = chroma == CRTFX_EGRESS_FIELD420_LEFT;
    const int wt[3] = {left ? 1 : 0, 2, left ? 1 : 2};
    const int top[4] = {left ? 3 : 0, left ? 7 : 8, left ? 5 : 8, left ? 1 : 0}, bottom[4] = {left ? 1 : 0, left ? 5 : 8, left ? 7 : 8, left ? 3 : 0};
    for (int i = 0; i < 3; ++i) a.wt[i] = wt[i];
    for (int i = 0; i < 4; ++i) { a.vt[i] = top[i]; a.vb[i] = bottom[i]; }
}

// the admission rule of crtfx_egress_field420.h for one row: K + N * X >= 0 and K + P * X < limit
bool row_fits(const int32_t* row, long long konst, long long x, long long limit) {
    long long pos = 0, neg = 0;
    for (int i = 0; i < 3; ++i) { if (row[i] > 0) pos += row[i]; else neg += row[i]; }
    return konst + neg * x >= 0 && konst + pos * x < limit;
}

}  // namespace

extern "C" {

const char* crtfx_egress_field420_last_error(const crtfx_egress_field420* p) { return p ? p->err.c_str() : create_err<crtfx_egress_field420>().c_str(); }

int crtfx_egress_field420_create(int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, crtfx_egress_field420** out_plan) {
    using H = crtfx_egress_field420;
    if (const int rc = begin_create(out_plan)) return rc;
    if (h >= 1 && h < 4) return fail<H>(nullptr, CRTFX_E_INVALID, "height %d is below 4: each field needs a chroma row of its own", h);
    if (h >= 1 && (h & 3))
        return fail<H>(nullptr, CRTFX_E_INVALID, "height %d is not a multiple of 4: each field of an interlaced 4:2:0 frame needs whole pairs of luma rows under its chroma rows", h);
    const bool known = layout >= CRTFX_FIELD420_YUV420P && layout <= CRTFX_FIELD420_P010LE;
    const bool deep = known && is_deep(layout);
    if (known && pix_fmt == (deep ? CRTFX_PIX_U8 : CRTFX_PIX_F16))
        return fail<H>(nullptr, CRTFX_E_UNSUPPORTED, deep ? "only half RGB frames are converted to %s (uint8 frames take an 8-bit layout)"
                                                           : "only uint8 RGB frames are converted to %s (half frames take a 10-bit layout)", LAYOUT_NAMES[layout]);
    if (const int rc = check_create<H>(pix_fmt, known ? (deep ? CRTFX_PIX_F16 : CRTFX_PIX_U8) : pix_fmt == CRTFX_PIX_F16 ? CRTFX_PIX_F16 : CRTFX_PIX_U8,
                                       h, w, layout, known, m, off, deep ? 1023 : 255)) return rc;
    // the admission rules of crtfx_egress_field420.h: X is the largest weighted sum of per-pixel codes
    const long long top = deep ? 1020 : 255, x = 64 * top;
    const long long k[3] = {((long long)off[0] << SH) + (1LL << (SH - 1)), ((long long)off[1] << CSH) + (1LL << (CSH - 1)), ((long long)off[2] << CSH) + (1LL << (CSH - 1))};
    const long long limit = deep ? 1LL << 32 : 1LL << 31;
    if (!row_fits(m, k[0], top, 1LL << 31) || !row_fits(m + 3, k[1], x, limit) || !row_fits(m + 6, k[2], x, limit))
        return fail<H>(nullptr, CRTFX_E_INVALID, deep ? "the matrix lets an accumulator leave [0, 2^32) (Y: [0, 2^31))" : "the matrix lets an accumulator leave [0, 2^31)");
    H* p = nullptr;
    if (const int rc = new_plan(true, device, layout, h, w, m, &p)) return rc;
    Args& a = p->args;
    a.ch = h / 2; a.cw = (w + 1) / 2;
    for (int i = 0; i < 3; ++i) a.k[i] = (unsigned)k[i];
    set_chroma(p, CRTFX_EGRESS_FIELD420_CENTER);
    const size_t luma_n = (size_t)h * w, chroma_n = 2 * (size_t)a.ch * a.cw;
    p->frame_bytes = (luma_n + chroma_n) * (deep ? 2 : 1);
    p->rgb_bytes = luma_n * (deep ? 6 : 3);
    Unit::note_plan(p, vec_fits(p, nullptr, 0, nullptr, 0, 1), 0);
    *out_plan = p;
    return CRTFX_OK;
}

int crtfx_egress_field420_destroy(crtfx_egress_field420* p) { return destroy(p); }
size_t crtfx_egress_field420_frame_bytes(const crtfx_egress_field420* p) { return p ? p->frame_bytes : 0; }

int crtfx_egress_field420_set_option(crtfx_egress_field420* p, int option, int value) {
    if (!p || option != CRTFX_EGRESS_FIELD420_OPT_CHROMA) return set_option<Unit>(p, option, value);
    if (value != CRTFX_EGRESS_FIELD420_CENTER && value != CRTFX_EGRESS_FIELD420_LEFT) return fail(p, CRTFX_E_INVALID, "CHROMA takes 0 (center) or 1 (left), got %d", value);
    set_chroma(p, value);
    Unit::note_plan(p, vec_fits(p, nullptr, 0, nullptr, 0, 1), 0);
    return CRTFX_OK;
}

int crtfx_egress_field420_last_plan(crtfx_egress_field420* p, char* buf, size_t n) { return last_plan(p, buf, n); }
int crtfx_egress_field420_run(crtfx_egress_field420* p, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream) {
    return run_frames<Unit>(p, src_base, src_stride_bytes, dst_base, dst_stride_bytes, n, stream);
}

}  // extern "C"
