// crtfx_field420.hip — the field-paired 4:2:0 source stage of libcrtfx.so (include/crtfx_field420.h): yuv420p / nv12 / yuv420p10le / p010le ->
// RGB with every luma row taking chroma from rows of its own field only.  A translation unit of its own: it shares no kernel, table or
// handle with the effect chain or the other stages; the loaders are those of crtfx_sited.hip's 4:2:0 layouts, restated here because that
// unit's builds are held to their register counts.  The host code around the kernels (checks, frame-group loop, error strings) is the
// skeleton of crtfx_stage_host.h; the chroma option is this unit's own.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "crtfx_field420.h"
#include "crtfx_stage_host.h"

namespace crtfx_field420_impl {

constexpr int BLOCK = 256;
constexpr int SH = 16;                          // fractional bits of the matrix; the interpolation weights (sum 32) carry five more
constexpr int WSH = 5;
constexpr int GENERAL = 0, VEC = 1;             // the PATH template argument; LAYOUT is a crtfx_field420_layout

struct Args {
    const uint8_t* src; size_t src_stride;
    uint8_t* dst; size_t dst_stride;
    int h, w, ch, cw;                           // ch = h / 2 chroma rows, which are also the luma rows of one field
    int m[9];                                   // rows R, G, B over the columns Y, U, V
    int k[3];                                   // off0, 32 * off1, 32 * off2
    int we[2], wo[2];                           // (near, far) horizontal weights of an even and an odd column, in quarters
    int vn[4], vf[4];                           // (near, far) vertical weights in eighths of [2 * field + (field row & 1)]
};

// unsigned dwords at 4-byte alignment: the widest access the vec path's rule (crtfx_field420.h) guarantees
struct __attribute__((packed, aligned(4))) U2 { unsigned v[2]; };
struct __attribute__((packed, aligned(4))) U4 { unsigned v[4]; };
struct __attribute__((packed, aligned(4))) U6 { unsigned v[6]; };
struct __attribute__((packed, aligned(4))) U12 { unsigned v[12]; };

template <int LAYOUT> struct Traits {
    static constexpr bool deep = LAYOUT == CRTFX_FIELD420_YUV420P10LE || LAYOUT == CRTFX_FIELD420_P010LE;
    static constexpr bool p010 = LAYOUT == CRTFX_FIELD420_P010LE;
    static constexpr bool semi = LAYOUT == CRTFX_FIELD420_NV12 || p010;                                    // one plane of (U, V) pairs
    static constexpr unsigned top = deep ? 1020u : 255u;       // the largest output code (10-bit: quarter codes)
};

// the 10-bit sample of a 16-bit word: bits outside the sample are ignored
template <bool P010> __device__ __forceinline__ int sample(unsigned word16) { return (int)(P010 ? (word16 & 0xFFFFu) >> 6 : word16 & 1023u); }

// clamp(acc >> 21, 0, top) of a signed accumulator in the form of the other stages (crtfx_unpack.hip says why): lower clamp on the
// accumulator, a LOGICAL shift of the non-negative rest, an unsigned minimum.
template <unsigned TOP, int SHIFT> __device__ __forceinline__ unsigned clamp_code(int acc) { return min((unsigned)max(acc, 0) >> SHIFT, TOP); }

// the half bit pattern of quarter code q, q / 4 on the 0..255 scale: exact, every quarter code is a half (no rounding occurs)
__device__ __forceinline__ unsigned half_bits(unsigned q) { return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)((float)q * 0.25f)); }

// a * b where both factors lie inside 24 signed bits and the product inside 32: the full-rate multiply (v_mul_i32_i24 / v_mad_i32_i24),
// where the 32 x 32 one issues at a quarter of the rate.  Every product below is of that kind: weights up to 8, samples and blends up to
// 32 * 1023, and matrix entries that create's rules hold below 2^22 with every sum of products inside int32.
__device__ __forceinline__ int mul24(int a, int b) { return __mul24(a, b); }

// The three output codes of one pixel.  hu / hv: the horizontal blends hn * C[.][cx] + hf * C[.][cxf] of the pixel's column in each chroma
// row the lane holds; row 1 of three is the own chroma row of the field, row 0 the one above and row 2 the one below; `far` names the far
// row of this luma row, vn / vf the vertical weights.  8-bit: the accumulator of crtfx_field420.h in int32 (create's rule).  10-bit: that
// accumulator does not fit; the header's rearrangement — whole 32nds of the chroma terms beside the luma term, the remainders apart,
// floor((32 S + R) / 2^21) = floor((S + floor(R / 32)) / 2^16) — gives the same code from int32 sums.
template <int LAYOUT>
__device__ __forceinline__ void pixel(const Args& a, int luma, const int (&hu)[3], const int (&hv)[3], int vn, int vf, int far, unsigned out[3]) {
    using T = Traits<LAYOUT>;
    const int d = mul24(vn, hu[1]) + mul24(vf, hu[far]) - a.k[1], e = mul24(vn, hv[1]) + mul24(vf, hv[far]) - a.k[2];
    const int c = luma - a.k[0];
    if (T::deep) {
        const int dq = d >> WSH, dr = d & ((1 << WSH) - 1), eq = e >> WSH, er = e & ((1 << WSH) - 1);      // d = 32 dq + dr, floor and remainder
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int s = mul24(a.m[3 * k], c) + mul24(a.m[3 * k + 1], dq) + mul24(a.m[3 * k + 2], eq);
            const int r = mul24(a.m[3 * k + 1], dr) + mul24(a.m[3 * k + 2], er) + (1 << (SH + WSH - 1));
            out[k] = clamp_code<T::top, SH>(s + (r >> WSH));
        }
    } else {
        const int c32 = c * (1 << WSH);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            out[k] = clamp_code<T::top, SH + WSH>(mul24(a.m[3 * k], c32) + mul24(a.m[3 * k + 1], d) + mul24(a.m[3 * k + 2], e) + (1 << (SH + WSH - 1)));
    }
}

// ---- general: one lane = one chroma sample position of a field and the (up to) 2 x 2 pixels of that field under it; bytes (8-bit) or
// 16-bit words (10-bit) only, any size ----

template <int LAYOUT>
__device__ __forceinline__ int luma_at(const uint8_t* fsrc, const Args& a, int y, int x) {
    using T = Traits<LAYOUT>;
    if (T::deep) return sample<T::p010>(reinterpret_cast<const uint16_t*>(fsrc)[(size_t)y * a.w + x]);
    return fsrc[(size_t)y * a.w + x];
}

// frame chroma row r, column cx
template <int LAYOUT>
__device__ __forceinline__ void chroma_at(const uint8_t* fsrc, const Args& a, int r, int cx, int& u, int& v) {
    using T = Traits<LAYOUT>;
    const size_t o = (size_t)r * a.cw + cx, plane = (size_t)a.ch * a.cw;
    if (T::deep) {
        const uint16_t* cb = reinterpret_cast<const uint16_t*>(fsrc) + (size_t)a.h * a.w;
        if (T::semi) { u = sample<T::p010>(cb[2 * o]); v = sample<T::p010>(cb[2 * o + 1]); }
        else { u = sample<T::p010>(cb[o]); v = sample<T::p010>(cb[plane + o]); }
    } else {
        const uint8_t* cb = fsrc + (size_t)a.h * a.w;
        if (T::semi) { u = cb[2 * o]; v = cb[2 * o + 1]; }
        else { u = cb[o]; v = cb[plane + o]; }
    }
}

// ---- vec (w % 8 == 0, 4-byte-aligned frame bases): one lane = 8 columns of two rows of one field; consecutive lanes, consecutive column
// blocks.  The chroma samples beside the lane's four are read with one narrow load each, at clamped indices. ----

// the 8 luma samples of frame row y, column block bx
template <int LAYOUT>
__device__ __forceinline__ void luma_block(const uint8_t* fsrc, const Args& a, int y, int bx, int (&l)[8]) {
    using T = Traits<LAYOUT>;
    if (T::deep) {
        const U4 d = *reinterpret_cast<const U4*>(fsrc + (size_t)y * a.w * 2 + (size_t)bx * 16);
#pragma unroll
        for (int p = 0; p < 8; ++p) l[p] = sample<T::p010>(d.v[p >> 1] >> (16 * (p & 1)));
    } else {
        const U2 d = *reinterpret_cast<const U2*>(fsrc + (size_t)y * a.w + (size_t)bx * 8);
#pragma unroll
        for (int p = 0; p < 8; ++p) l[p] = (int)((d.v[p >> 2] >> (8 * (p & 3))) & 255u);
    }
}

// frame chroma row r: u[1..4], v[1..4] = the lane's four samples, [0] = sample cl to their left, [5] = sample cr to their right (clamped by the caller)
template <int LAYOUT>
__device__ __forceinline__ void chroma_block(const uint8_t* fsrc, const Args& a, int r, int bx, int cl, int cr, int (&u)[6], int (&v)[6]) {
    using T = Traits<LAYOUT>;
    if (T::deep && T::semi) {                   // u0 v0 | u1 v1 | u2 v2 | u3 v3: one chroma sample per dword
        const uint8_t* row = fsrc + (size_t)a.h * a.w * 2 + (size_t)r * a.w * 2;
        const U4 d = *reinterpret_cast<const U4*>(row + (size_t)bx * 16);
        const unsigned dl = *reinterpret_cast<const unsigned*>(row + (size_t)cl * 4), dr = *reinterpret_cast<const unsigned*>(row + (size_t)cr * 4);
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const unsigned uv = q == 0 ? dl : q == 5 ? dr : d.v[q - 1];
            u[q] = sample<T::p010>(uv); v[q] = sample<T::p010>(uv >> 16);
        }
    } else if (T::deep) {
        const uint8_t* ur = fsrc + ((size_t)a.h * a.w + (size_t)r * a.cw) * 2;
        const uint8_t* vr = ur + (size_t)a.ch * a.cw * 2;
        const U2 du = *reinterpret_cast<const U2*>(ur + (size_t)bx * 8), dv = *reinterpret_cast<const U2*>(vr + (size_t)bx * 8);
#pragma unroll
        for (int q = 0; q < 4; ++q) { u[q + 1] = sample<T::p010>(du.v[q >> 1] >> (16 * (q & 1))); v[q + 1] = sample<T::p010>(dv.v[q >> 1] >> (16 * (q & 1))); }
        const uint16_t* uw = reinterpret_cast<const uint16_t*>(ur);
        const uint16_t* vw = reinterpret_cast<const uint16_t*>(vr);
        u[0] = sample<T::p010>(uw[cl]); u[5] = sample<T::p010>(uw[cr]); v[0] = sample<T::p010>(vw[cl]); v[5] = sample<T::p010>(vw[cr]);
    } else if (T::semi) {                       // u0 v0 u1 v1 | u2 v2 u3 v3
        const uint8_t* row = fsrc + (size_t)a.h * a.w + (size_t)r * a.w;
        const U2 d = *reinterpret_cast<const U2*>(row + (size_t)bx * 8);
        const unsigned dl = *reinterpret_cast<const uint16_t*>(row + (size_t)cl * 2), dr = *reinterpret_cast<const uint16_t*>(row + (size_t)cr * 2);
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const unsigned uv = q == 0 ? dl : q == 5 ? dr : d.v[(q - 1) >> 1] >> (16 * ((q - 1) & 1));
            u[q] = (int)(uv & 255u); v[q] = (int)((uv >> 8) & 255u);
        }
    } else {
        const uint8_t* ur = fsrc + (size_t)a.h * a.w + (size_t)r * a.cw;
        const uint8_t* vr = ur + (size_t)a.ch * a.cw;
        const unsigned du = *reinterpret_cast<const unsigned*>(ur + (size_t)bx * 4), dv = *reinterpret_cast<const unsigned*>(vr + (size_t)bx * 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) { u[q + 1] = (int)((du >> (8 * q)) & 255u); v[q + 1] = (int)((dv >> (8 * q)) & 255u); }
        u[0] = ur[cl]; u[5] = ur[cr]; v[0] = vr[cl]; v[5] = vr[cr];
    }
}

// Lane rows: (ch + 1) / 2 per field, interleaved — lane row R serves field f = R & 1, field chroma row i = R >> 1, that is the luma rows
// 4 i + f and 4 i + 2 + f (the second one only where it is inside the frame: with h % 4 == 2 the last lane row of either field has one).
template <int LAYOUT, int PATH>
__global__ __launch_bounds__(BLOCK) void k_unpack_field420(Args a) {
    using T = Traits<LAYOUT>;
    const uint8_t* fsrc = a.src + (size_t)blockIdx.z * a.src_stride;
    uint8_t* fdst = a.dst + (size_t)blockIdx.z * a.dst_stride;
    const int idx = blockIdx.x * BLOCK + threadIdx.x;
    const int per_row = PATH == VEC ? a.w >> 3 : a.cw;
    const int lane_rows = 2 * ((a.ch + 1) >> 1);
    if (idx >= lane_rows * per_row) return;
    const int R = idx / per_row, bx = idx - R * per_row;       // general: bx is the chroma column
    const int f = R & 1, i = R >> 1;
    const int y0 = 4 * i + f;
    const bool second = y0 + 2 < a.h;
    // the frame chroma rows of the field: above, own, below, each clamped to the field's rows [0, n_f - 1]
    const int last = ((a.ch + 1 - f) >> 1) - 1;
    const int rr[3] = {2 * min(max(i - 1, 0), last) + f, 2 * min(i, last) + f, 2 * min(i + 1, last) + f};
    // the vertical weights of the lane's two rows
    const int vn[2] = {f ? a.vn[2] : a.vn[0], f ? a.vn[3] : a.vn[1]}, vf[2] = {f ? a.vf[2] : a.vf[0], f ? a.vf[3] : a.vf[1]};
    if (PATH == VEC) {
        const int cl = max(4 * bx - 1, 0), cr = min(4 * bx + 4, a.cw - 1);
        int u[3][6], v[3][6], l[2][8];
#pragma unroll
        for (int j = 0; j < 3; ++j) chroma_block<LAYOUT>(fsrc, a, rr[j], bx, cl, cr, u[j], v[j]);
        luma_block<LAYOUT>(fsrc, a, y0, bx, l[0]);
        luma_block<LAYOUT>(fsrc, a, second ? y0 + 2 : y0, bx, l[1]);
        unsigned code[2][24];
#pragma unroll
        for (int p = 0; p < 8; ++p) {           // column p: own sample q + 1; far sample q (even p) or q + 2 (odd p)
            const int q = (p >> 1) + 1, fq = (p & 1) ? q + 1 : q - 1;
            const int wn = (p & 1) ? a.wo[0] : a.we[0], wf = (p & 1) ? a.wo[1] : a.we[1];
            int hu[3], hv[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) { hu[j] = mul24(wn, u[j][q]) + mul24(wf, u[j][fq]); hv[j] = mul24(wn, v[j][q]) + mul24(wf, v[j][fq]); }
#pragma unroll
            for (int r = 0; r < 2; ++r) pixel<LAYOUT>(a, l[r][p], hu, hv, vn[r], vf[r], r ? 2 : 0, &code[r][3 * p]);
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r == 1 && !second) break;
            if (T::deep) {
                U12 o;
#pragma unroll
                for (int t = 0; t < 12; ++t) o.v[t] = half_bits(code[r][2 * t]) | (half_bits(code[r][2 * t + 1]) << 16);
                *reinterpret_cast<U12*>(fdst + (size_t)(y0 + 2 * r) * a.w * 6 + (size_t)bx * 48) = o;
            } else {
                U6 o;
#pragma unroll
                for (int t = 0; t < 6; ++t) o.v[t] = code[r][4 * t] | (code[r][4 * t + 1] << 8) | (code[r][4 * t + 2] << 16) | (code[r][4 * t + 3] << 24);
                *reinterpret_cast<U6*>(fdst + (size_t)(y0 + 2 * r) * a.w * 3 + (size_t)bx * 24) = o;
            }
        }
    } else {
        const int x0 = 2 * bx;
        const bool right = x0 + 1 < a.w;
        const int cc[3] = {max(bx - 1, 0), bx, min(bx + 1, a.cw - 1)};
        int u[3][3], v[3][3];                   // [chroma row][left, own, right]
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int t = 0; t < 3; ++t) chroma_at<LAYOUT>(fsrc, a, rr[j], cc[t], u[j][t], v[j][t]);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r == 1 && !second) break;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                if (e == 1 && !right) break;
                const int wn = e ? a.wo[0] : a.we[0], wf = e ? a.wo[1] : a.we[1];
                int hu[3], hv[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) { hu[j] = mul24(wn, u[j][1]) + mul24(wf, u[j][2 * e]); hv[j] = mul24(wn, v[j][1]) + mul24(wf, v[j][2 * e]); }
                unsigned code[3];
                pixel<LAYOUT>(a, luma_at<LAYOUT>(fsrc, a, y0 + 2 * r, x0 + e), hu, hv, vn[r], vf[r], r ? 2 : 0, code);
                const size_t o = ((size_t)(y0 + 2 * r) * a.w + x0 + e) * 3;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    if (T::deep) reinterpret_cast<uint16_t*>(fdst)[o + k] = (uint16_t)half_bits(code[k]);
                    else fdst[o + k] = (uint8_t)code[k];
                }
            }
        }
    }
}

}  // namespace crtfx_field420_impl

using namespace crtfx_field420_impl;
using namespace crtfx_stage;

struct crtfx_field420 : StagePlan { Args args{}; int chroma = CRTFX_FIELD420_REPLICATE; };        // `egress` stays false

namespace {

static_assert(SH == MATRIX_SH, "the matrices are the other stages'");

const char* const LAYOUT_NAMES[4] = {"yuv420p", "nv12", "yuv420p10le", "p010le"};
const char* const CHROMA_NAMES[3] = {"replicate", "left", "center"};
bool is_deep(int layout) { return layout == CRTFX_FIELD420_YUV420P10LE || layout == CRTFX_FIELD420_P010LE; }

template <int LAYOUT>
void launch_layout(bool vec, dim3 grid, hipStream_t st, const Args& a) {
    if (vec) hipLaunchKernelGGL((k_unpack_field420<LAYOUT, VEC>), grid, dim3(BLOCK), 0, st, a);
    else hipLaunchKernelGGL((k_unpack_field420<LAYOUT, GENERAL>), grid, dim3(BLOCK), 0, st, a);
}

struct Unit {
    static constexpr int block = BLOCK, force_option = CRTFX_FIELD420_OPT_FORCE_GENERAL;
    static const char* name(bool) { return "field420"; }
    static void note_plan(crtfx_field420* p, bool vec, int frames) {
        snprintf(p->plan, sizeof p->plan, "field420=k_unpack_field420<%s,%s>;chroma=%s;frames=%d", LAYOUT_NAMES[p->layout], vec ? "vec" : "general",
                 CHROMA_NAMES[p->chroma], frames);
    }
    static int check_alignment(crtfx_field420* p, const void* src_base, size_t src_stride_bytes, const void* dst_base, size_t dst_stride_bytes) {
        if (is_deep(p->layout) && ((reinterpret_cast<uintptr_t>(src_base) | reinterpret_cast<uintptr_t>(dst_base) | src_stride_bytes | dst_stride_bytes) & 1u))
            return fail(p, CRTFX_E_INVALID, "an odd frame base or stride: 16-bit samples need 2-byte alignment");
        return CRTFX_OK;                                                                                  // bytes: any base, any stride
    }
    // two fields of (ch + 1) / 2 lane rows: at most 16384 * 16384
    static int items(const Args& a, bool vec) { return 2 * ((a.ch + 1) / 2) * (vec ? a.w >> 3 : a.cw); }
    static void launch(const crtfx_field420* p, bool vec, dim3 grid, hipStream_t st, const Args& a) {
        switch (p->layout) {
            case CRTFX_FIELD420_NV12: launch_layout<CRTFX_FIELD420_NV12>(vec, grid, st, a); break;
            case CRTFX_FIELD420_YUV420P10LE: launch_layout<CRTFX_FIELD420_YUV420P10LE>(vec, grid, st, a); break;
            case CRTFX_FIELD420_P010LE: launch_layout<CRTFX_FIELD420_P010LE>(vec, grid, st, a); break;
            default: launch_layout<CRTFX_FIELD420_YUV420P>(vec, grid, st, a); break;
        }
    }
};

// the weights of crtfx_field420.h: horizontal in quarters, vertical in eighths of [2 * field + (field row & 1)]
void set_chroma(crtfx_field420* p, int chroma) {
    Args& a = p->args;
    p->chroma = chroma;
    const bool rep = chroma == CRTFX_FIELD420_REPLICATE;
    if (chroma == CRTFX_FIELD420_CENTER) { a.we[0] = 3; a.we[1] = 1; a.wo[0] = 3; a.wo[1] = 1; }
    else if (chroma == CRTFX_FIELD420_LEFT) { a.we[0] = 4; a.we[1] = 0; a.wo[0] = 2; a.wo[1] = 2; }
    else { a.we[0] = 4; a.we[1] = 0; a.wo[0] = 4; a.wo[1] = 0; }
    const int near[4] = {7, 5, 5, 7};           // top field: even, odd field row; bottom field: even, odd
    for (int i = 0; i < 4; ++i) { a.vn[i] = rep ? 8 : near[i]; a.vf[i] = 8 - a.vn[i]; }
}

long long mag(int32_t x) { return x < 0 ? -(long long)x : (long long)x; }

// the admission rules of crtfx_field420.h: the 8-bit accumulator, and the two int32 sums of the 10-bit rearrangement
bool row_fits(const int32_t* row, bool deep) {
    const long long sum = mag(row[0]) + mag(row[1]) + mag(row[2]);
    return deep ? sum * 1024 + (1LL << (SH - 1)) < (1LL << 31) : sum * 255 * 32 + (1LL << (SH + WSH - 1)) < (1LL << 31);
}

}  // namespace

extern "C" {

const char* crtfx_field420_last_error(const crtfx_field420* p) { return p ? p->err.c_str() : create_err<crtfx_field420>().c_str(); }

int crtfx_field420_create(int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, crtfx_field420** out_plan) {
    using H = crtfx_field420;
    if (const int rc = begin_create(out_plan)) return rc;
    if (h & 1) return fail<H>(nullptr, CRTFX_E_INVALID, "height %d is odd: the two fields of an interlaced 4:2:0 frame have the same number of rows", h);
    if (h < 4) return fail<H>(nullptr, CRTFX_E_INVALID, "height %d is below 4: each field needs a chroma row of its own", h);
    const bool known = layout >= CRTFX_FIELD420_YUV420P && layout <= CRTFX_FIELD420_P010LE;
    const bool deep = known && is_deep(layout);
    if (known && pix_fmt == (deep ? CRTFX_PIX_U8 : CRTFX_PIX_F16))
        return fail<H>(nullptr, CRTFX_E_UNSUPPORTED, deep ? "only half RGB frames are written from %s (uint8 frames take an 8-bit layout)"
                                                           : "only uint8 RGB frames are written from %s (half frames take a 10-bit layout)", LAYOUT_NAMES[layout]);
    if (const int rc = check_create<H>(pix_fmt, known ? (deep ? CRTFX_PIX_F16 : CRTFX_PIX_U8) : pix_fmt == CRTFX_PIX_F16 ? CRTFX_PIX_F16 : CRTFX_PIX_U8,
                                       h, w, layout, known, m, off, deep ? 1023 : 255)) return rc;
    if (!(row_fits(m, deep) && row_fits(m + 3, deep) && row_fits(m + 6, deep)))
        return fail<H>(nullptr, CRTFX_E_INVALID, "the matrix lets an accumulator leave int32");
    H* p = nullptr;
    if (const int rc = new_plan(false, device, layout, h, w, m, &p)) return rc;
    Args& a = p->args;
    a.ch = h / 2; a.cw = (w + 1) / 2;
    a.k[0] = off[0]; a.k[1] = off[1] << WSH; a.k[2] = off[2] << WSH;
    set_chroma(p, CRTFX_FIELD420_REPLICATE);
    const size_t luma = (size_t)h * w, chroma = 2 * (size_t)a.ch * a.cw;
    p->frame_bytes = (luma + chroma) * (deep ? 2 : 1);
    p->rgb_bytes = luma * (deep ? 6 : 3);
    Unit::note_plan(p, vec_fits(p, nullptr, 0, nullptr, 0, 1), 0);
    *out_plan = p;
    return CRTFX_OK;
}

int crtfx_field420_destroy(crtfx_field420* p) { return destroy(p); }
size_t crtfx_field420_frame_bytes(const crtfx_field420* p) { return p ? p->frame_bytes : 0; }

int crtfx_field420_set_option(crtfx_field420* p, int option, int value) {
    if (!p || option != CRTFX_FIELD420_OPT_CHROMA) return set_option<Unit>(p, option, value);
    if (value < CRTFX_FIELD420_REPLICATE || value > CRTFX_FIELD420_CENTER)
        return fail(p, CRTFX_E_INVALID, "CHROMA takes 0 (replicate), 1 (left) or 2 (center), got %d", value);
    set_chroma(p, value);
    Unit::note_plan(p, vec_fits(p, nullptr, 0, nullptr, 0, 1), 0);
    return CRTFX_OK;
}

int crtfx_field420_last_plan(crtfx_field420* p, char* buf, size_t n) { return last_plan(p, buf, n); }
int crtfx_field420_run(crtfx_field420* p, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream) {
    return run_frames<Unit>(p, src_base, src_stride_bytes, dst_base, dst_stride_bytes, n, stream);
}

}  // extern "C"
