// crtfx_sited.hip — the sited source stage of libcrtfx.so (include/crtfx_sited.h): the seven sub-sampled source formats of crtfx_unpack_*,
// crtfx_unpack422_* and crtfx_unpack10_* -> RGB with chroma interpolated at a stated siting instead of replicated.  A translation unit of
// its own: it shares no kernel, table or handle with the effect chain or the other stages.  The host code around the kernels (checks,
// frame-group loop, error strings) is the skeleton of crtfx_stage_host.h; the siting option is this unit's own.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "crtfx_sited.h"
#include "crtfx_stage_host.h"

namespace crtfx_sited_impl {

constexpr int BLOCK = 256;
constexpr int SH = 16;                          // fractional bits of the matrix; the interpolation weights (sum 16) carry four more
constexpr int WSH = 4;
constexpr int GENERAL = 0, VEC = 1;             // the PATH template argument; LAYOUT is a crtfx_sited_layout

struct Args {
    const uint8_t* src; size_t src_stride;
    uint8_t* dst; size_t dst_stride;
    int h, w, rows, cw;                         // rows: chroma rows, (h + 1) / 2 for 4:2:0 and h for 4:2:2
    int m[9];                                   // rows R, G, B over the columns Y, U, V
    int k[3];                                   // off0, 16 * off1, 16 * off2
    int we[2], wo[2];                           // (near, far) horizontal weights of an even and an odd column: the siting
};

// unsigned dwords at 4-byte alignment: the widest access the vec path's rule (crtfx_sited.h) guarantees
struct __attribute__((packed, aligned(4))) U2 { unsigned v[2]; };
struct __attribute__((packed, aligned(4))) U4 { unsigned v[4]; };
struct __attribute__((packed, aligned(4))) U6 { unsigned v[6]; };
struct __attribute__((packed, aligned(4))) U12 { unsigned v[12]; };

template <int LAYOUT> struct Traits {
    static constexpr bool deep = LAYOUT == CRTFX_SITED_YUV420P10LE || LAYOUT == CRTFX_SITED_P010LE;
    static constexpr bool p010 = LAYOUT == CRTFX_SITED_P010LE;
    static constexpr bool v420 = LAYOUT == CRTFX_SITED_YUV420P || LAYOUT == CRTFX_SITED_NV12 || deep;     // chroma rows are halved too
    static constexpr bool semi = LAYOUT == CRTFX_SITED_NV12 || p010;                                      // one plane of (U, V) pairs
    static constexpr bool packed = LAYOUT == CRTFX_SITED_YUYV422 || LAYOUT == CRTFX_SITED_UYVY422;        // macropixels
    static constexpr int NR = v420 ? 2 : 1;     // luma rows of a lane
    static constexpr int NC = v420 ? 3 : 1;     // chroma rows a lane reads: above, own, below
    // byte positions inside a packed macropixel: yuyv422 = Y0 U Y1 V, uyvy422 = U Y0 V Y1
    static constexpr int Y0 = LAYOUT == CRTFX_SITED_YUYV422 ? 0 : 1, Y1 = Y0 + 2, U = LAYOUT == CRTFX_SITED_YUYV422 ? 1 : 0, V = U + 2;
    static constexpr unsigned top = deep ? 1020u : 255u;       // the largest output code (10-bit: quarter codes)
};

// the 10-bit sample of a 16-bit word: bits outside the sample are ignored
template <bool P010> __device__ __forceinline__ int sample(unsigned word16) { return (int)(P010 ? (word16 & 0xFFFFu) >> 6 : word16 & 1023u); }

// clamp(acc >> 20, 0, top) of a signed accumulator in the form of the other stages (crtfx_unpack.hip says why): lower clamp on the
// accumulator, a LOGICAL shift of the non-negative rest, an unsigned minimum.
template <unsigned TOP> __device__ __forceinline__ unsigned clamp_code(int acc) { return min((unsigned)max(acc, 0) >> (SH + WSH), TOP); }

// the half bit pattern of quarter code q, q / 4 on the 0..255 scale: exact, every quarter code is a half (no rounding occurs)
__device__ __forceinline__ unsigned half_bits(unsigned q) { return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)((float)q * 0.25f)); }

// The three output codes of one pixel.  n / f: the near (own) and far chroma sample of the pixel's column in each chroma row the lane
// holds, wn / wf their horizontal weights; row 1 of three is the own chroma row, row 0 the one above and row 2 the one below; `far` names
// the far row of this luma row.  8-bit: one int32 accumulator (create's rule).  10-bit: the luma and the chroma part each fit int32, their
// sum may not: a saturating add, whose saturation points lie outside [0, 1020 << 20].
template <int LAYOUT>
__device__ __forceinline__ void pixel(const Args& a, int luma, const int (&un)[3], const int (&uf)[3], const int (&vn)[3], const int (&vf)[3],
                                      int wn, int wf, int far, unsigned out[3]) {
    using T = Traits<LAYOUT>;
    int du, dv;
    if (T::v420) {
        du = 3 * (wn * un[1] + wf * uf[1]) + (wn * un[far] + wf * uf[far]);
        dv = 3 * (wn * vn[1] + wf * vf[1]) + (wn * vn[far] + wf * vf[far]);
    } else {
        du = 4 * (wn * un[0] + wf * uf[0]);
        dv = 4 * (wn * vn[0] + wf * vf[0]);
    }
    const int c = (luma - a.k[0]) * (1 << WSH), d = du - a.k[1], e = dv - a.k[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int t = a.m[3 * k + 1] * d + a.m[3 * k + 2] * e + (1 << (SH + WSH - 1));
        const int acc = T::deep ? __builtin_elementwise_add_sat(a.m[3 * k] * c, t) : a.m[3 * k] * c + t;
        out[k] = clamp_code<T::top>(acc);
    }
}

// ---- general: one lane = one chroma sample and the (up to) 2 x 2 (4:2:0) or 2 x 1 (4:2:2) pixels under it; bytes (8-bit) or 16-bit words
// (10-bit) only, any size ----

template <int LAYOUT>
__device__ __forceinline__ int luma_at(const uint8_t* fsrc, const Args& a, int y, int x) {
    using T = Traits<LAYOUT>;
    if (T::deep) return sample<T::p010>(reinterpret_cast<const uint16_t*>(fsrc)[(size_t)y * a.w + x]);
    if (T::packed) return fsrc[((size_t)y * a.cw + (x >> 1)) * 4 + ((x & 1) ? T::Y1 : T::Y0)];       // the pad byte of an odd row is never asked for
    return fsrc[(size_t)y * a.w + x];
}

template <int LAYOUT>
__device__ __forceinline__ void chroma_at(const uint8_t* fsrc, const Args& a, int r, int cx, int& u, int& v) {
    using T = Traits<LAYOUT>;
    const size_t o = (size_t)r * a.cw + cx, plane = (size_t)a.rows * a.cw;
    if (T::deep) {
        const uint16_t* cb = reinterpret_cast<const uint16_t*>(fsrc) + (size_t)a.h * a.w;
        if (T::semi) { u = sample<T::p010>(cb[2 * o]); v = sample<T::p010>(cb[2 * o + 1]); }
        else { u = sample<T::p010>(cb[o]); v = sample<T::p010>(cb[plane + o]); }
    } else if (T::packed) {
        u = fsrc[4 * o + T::U]; v = fsrc[4 * o + T::V];
    } else {
        const uint8_t* cb = fsrc + (size_t)a.h * a.w;
        if (T::semi) { u = cb[2 * o]; v = cb[2 * o + 1]; }
        else { u = cb[o]; v = cb[plane + o]; }
    }
}

// ---- vec (w % 8 == 0, 4-byte-aligned frame bases): one lane = 8 columns of one (4:2:2) or two (4:2:0) rows; consecutive lanes, consecutive
// column blocks.  The chroma samples beside the lane's four are read with one narrow load each, at clamped indices. ----

// the 8 luma samples of row y, column block bx
template <int LAYOUT>
__device__ __forceinline__ void luma_block(const uint8_t* fsrc, const Args& a, int y, int bx, int (&l)[8]) {
    using T = Traits<LAYOUT>;
    if (T::deep || T::packed) {
        const U4 d = *reinterpret_cast<const U4*>(fsrc + (size_t)y * a.w * 2 + (size_t)bx * 16);
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            if (T::deep) l[p] = sample<T::p010>(d.v[p >> 1] >> (16 * (p & 1)));
            else l[p] = (int)((d.v[p >> 1] >> (8 * ((p & 1) ? T::Y1 : T::Y0))) & 255u);
        }
    } else {
        const U2 d = *reinterpret_cast<const U2*>(fsrc + (size_t)y * a.w + (size_t)bx * 8);
#pragma unroll
        for (int p = 0; p < 8; ++p) l[p] = (int)((d.v[p >> 2] >> (8 * (p & 3))) & 255u);
    }
}

// chroma row r: u[1..4], v[1..4] = the lane's four samples, [0] = sample cl to their left, [5] = sample cr to their right (clamped by the caller)
template <int LAYOUT>
__device__ __forceinline__ void chroma_block(const uint8_t* fsrc, const Args& a, int r, int bx, int cl, int cr, int (&u)[6], int (&v)[6]) {
    using T = Traits<LAYOUT>;
    if (T::packed) {
        const uint8_t* row = fsrc + (size_t)r * a.w * 2;
        const U4 d = *reinterpret_cast<const U4*>(row + (size_t)bx * 16);
        const unsigned dl = *reinterpret_cast<const unsigned*>(row + (size_t)cl * 4), dr = *reinterpret_cast<const unsigned*>(row + (size_t)cr * 4);
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const unsigned mp = q == 0 ? dl : q == 5 ? dr : d.v[q - 1];
            u[q] = (int)((mp >> (8 * T::U)) & 255u); v[q] = (int)((mp >> (8 * T::V)) & 255u);
        }
    } else if (T::deep && T::semi) {            // u0 v0 | u1 v1 | u2 v2 | u3 v3: one chroma sample per dword
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
        const uint8_t* vr = ur + (size_t)a.rows * a.cw * 2;
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
        const uint8_t* vr = ur + (size_t)a.rows * a.cw;
        const unsigned du = *reinterpret_cast<const unsigned*>(ur + (size_t)bx * 4), dv = *reinterpret_cast<const unsigned*>(vr + (size_t)bx * 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) { u[q + 1] = (int)((du >> (8 * q)) & 255u); v[q + 1] = (int)((dv >> (8 * q)) & 255u); }
        u[0] = ur[cl]; u[5] = ur[cr]; v[0] = vr[cl]; v[5] = vr[cr];
    }
}

template <int LAYOUT, int PATH>
__global__ __launch_bounds__(BLOCK) void k_unpack_sited(Args a) {
    using T = Traits<LAYOUT>;
    const uint8_t* fsrc = a.src + (size_t)blockIdx.z * a.src_stride;
    uint8_t* fdst = a.dst + (size_t)blockIdx.z * a.dst_stride;
    const int idx = blockIdx.x * BLOCK + threadIdx.x;
    const int per_row = PATH == VEC ? a.w >> 3 : a.cw;
    if (idx >= a.rows * per_row) return;
    const int cy = idx / per_row, bx = idx - cy * per_row;     // general: bx is the chroma column
    const int y0 = T::v420 ? 2 * cy : cy;
    const bool below = T::v420 && y0 + 1 < a.h;
    // the chroma rows: above (clamped), own, below (clamped); 4:2:2 has the own one only
    const int rr[3] = {T::v420 ? max(cy - 1, 0) : cy, cy, min(cy + 1, a.rows - 1)};
    if (PATH == VEC) {
        const int cl = max(4 * bx - 1, 0), cr = min(4 * bx + 4, a.cw - 1);
        int u[T::NC][6], v[T::NC][6], l[T::NR][8];
#pragma unroll
        for (int j = 0; j < T::NC; ++j) chroma_block<LAYOUT>(fsrc, a, rr[T::v420 ? j : 1], bx, cl, cr, u[j], v[j]);
        luma_block<LAYOUT>(fsrc, a, y0, bx, l[0]);
        if (T::v420) luma_block<LAYOUT>(fsrc, a, below ? y0 + 1 : y0, bx, l[T::NR - 1]);
        unsigned code[T::NR][24];
#pragma unroll
        for (int p = 0; p < 8; ++p) {           // column p: own sample q + 1; far sample q (even p) or q + 2 (odd p)
            const int q = (p >> 1) + 1, f = (p & 1) ? q + 1 : q - 1;
            int un[3], uf[3], vn[3], vf[3];
#pragma unroll
            for (int j = 0; j < T::NC; ++j) { un[j] = u[j][q]; uf[j] = u[j][f]; vn[j] = v[j][q]; vf[j] = v[j][f]; }
#pragma unroll
            for (int r = 0; r < T::NR; ++r)
                pixel<LAYOUT>(a, l[r][p], un, uf, vn, vf, (p & 1) ? a.wo[0] : a.we[0], (p & 1) ? a.wo[1] : a.we[1], r ? 2 : 0, &code[r][3 * p]);
        }
#pragma unroll
        for (int r = 0; r < T::NR; ++r) {
            if (r == 1 && !below) break;
            if (T::deep) {
                U12 o;
#pragma unroll
                for (int i = 0; i < 12; ++i) o.v[i] = half_bits(code[r][2 * i]) | (half_bits(code[r][2 * i + 1]) << 16);
                *reinterpret_cast<U12*>(fdst + (size_t)(y0 + r) * a.w * 6 + (size_t)bx * 48) = o;
            } else {
                U6 o;
#pragma unroll
                for (int i = 0; i < 6; ++i) o.v[i] = code[r][4 * i] | (code[r][4 * i + 1] << 8) | (code[r][4 * i + 2] << 16) | (code[r][4 * i + 3] << 24);
                *reinterpret_cast<U6*>(fdst + (size_t)(y0 + r) * a.w * 3 + (size_t)bx * 24) = o;
            }
        }
    } else {
        const int x0 = 2 * bx;
        const bool right = x0 + 1 < a.w;
        const int cc[3] = {max(bx - 1, 0), bx, min(bx + 1, a.cw - 1)};
        int u[3][3], v[3][3];                   // [chroma row][left, own, right]
#pragma unroll
        for (int j = 0; j < T::NC; ++j)
#pragma unroll
            for (int i = 0; i < 3; ++i) chroma_at<LAYOUT>(fsrc, a, rr[T::v420 ? j : 1], cc[i], u[j][i], v[j][i]);
#pragma unroll
        for (int r = 0; r < T::NR; ++r) {
            if (r == 1 && !below) break;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                if (e == 1 && !right) break;
                int un[3], uf[3], vn[3], vf[3];
#pragma unroll
                for (int j = 0; j < T::NC; ++j) { un[j] = u[j][1]; uf[j] = u[j][2 * e]; vn[j] = v[j][1]; vf[j] = v[j][2 * e]; }
                unsigned code[3];
                pixel<LAYOUT>(a, luma_at<LAYOUT>(fsrc, a, y0 + r, x0 + e), un, uf, vn, vf, e ? a.wo[0] : a.we[0], e ? a.wo[1] : a.we[1], r ? 2 : 0, code);
                const size_t o = ((size_t)(y0 + r) * a.w + x0 + e) * 3;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    if (T::deep) reinterpret_cast<uint16_t*>(fdst)[o + k] = (uint16_t)half_bits(code[k]);
                    else fdst[o + k] = (uint8_t)code[k];
                }
            }
        }
    }
}

}  // namespace crtfx_sited_impl

using namespace crtfx_sited_impl;
using namespace crtfx_stage;

struct crtfx_sited : StagePlan { Args args{}; int siting = CRTFX_SITED_LEFT; };        // `egress` stays false

namespace {

static_assert(SH == MATRIX_SH, "the matrices are the other stages'");

const char* const LAYOUT_NAMES[7] = {"yuv420p", "nv12", "yuv422p", "yuyv422", "uyvy422", "yuv420p10le", "p010le"};
bool is_deep(int layout) { return layout == CRTFX_SITED_YUV420P10LE || layout == CRTFX_SITED_P010LE; }
bool is_420(int layout) { return layout == CRTFX_SITED_YUV420P || layout == CRTFX_SITED_NV12 || is_deep(layout); }

template <int LAYOUT>
void launch_layout(bool vec, dim3 grid, hipStream_t st, const Args& a) {
    if (vec) hipLaunchKernelGGL((k_unpack_sited<LAYOUT, VEC>), grid, dim3(BLOCK), 0, st, a);
    else hipLaunchKernelGGL((k_unpack_sited<LAYOUT, GENERAL>), grid, dim3(BLOCK), 0, st, a);
}

struct Unit {
    static constexpr int block = BLOCK, force_option = CRTFX_SITED_OPT_FORCE_GENERAL;
    static const char* name(bool) { return "sited"; }
    static void note_plan(crtfx_sited* p, bool vec, int frames) {
        snprintf(p->plan, sizeof p->plan, "sited=k_unpack_sited<%s,%s>;siting=%s;frames=%d", LAYOUT_NAMES[p->layout], vec ? "vec" : "general",
                 p->siting == CRTFX_SITED_CENTER ? "center" : "left", frames);
    }
    static int check_alignment(crtfx_sited* p, const void* src_base, size_t src_stride_bytes, const void* dst_base, size_t dst_stride_bytes) {
        if (is_deep(p->layout) && ((reinterpret_cast<uintptr_t>(src_base) | reinterpret_cast<uintptr_t>(dst_base) | src_stride_bytes | dst_stride_bytes) & 1u))
            return fail(p, CRTFX_E_INVALID, "an odd frame base or stride: 16-bit samples need 2-byte alignment");
        return CRTFX_OK;                                                                                  // bytes: any base, any stride
    }
    static int items(const Args& a, bool vec) { return vec ? a.rows * (a.w >> 3) : a.rows * a.cw; }      // at most 32767 * 16384
    static void launch(const crtfx_sited* p, bool vec, dim3 grid, hipStream_t st, const Args& a) {
        switch (p->layout) {
            case CRTFX_SITED_NV12: launch_layout<CRTFX_SITED_NV12>(vec, grid, st, a); break;
            case CRTFX_SITED_YUV422P: launch_layout<CRTFX_SITED_YUV422P>(vec, grid, st, a); break;
            case CRTFX_SITED_YUYV422: launch_layout<CRTFX_SITED_YUYV422>(vec, grid, st, a); break;
            case CRTFX_SITED_UYVY422: launch_layout<CRTFX_SITED_UYVY422>(vec, grid, st, a); break;
            case CRTFX_SITED_YUV420P10LE: launch_layout<CRTFX_SITED_YUV420P10LE>(vec, grid, st, a); break;
            case CRTFX_SITED_P010LE: launch_layout<CRTFX_SITED_P010LE>(vec, grid, st, a); break;
            default: launch_layout<CRTFX_SITED_YUV420P>(vec, grid, st, a); break;
        }
    }
};

void set_siting(crtfx_sited* p, int siting) {
    Args& a = p->args;
    p->siting = siting;
    if (siting == CRTFX_SITED_CENTER) { a.we[0] = 3; a.we[1] = 1; a.wo[0] = 3; a.wo[1] = 1; }
    else { a.we[0] = 4; a.we[1] = 0; a.wo[0] = 2; a.wo[1] = 2; }
}

long long mag(int32_t x) { return x < 0 ? -(long long)x : (long long)x; }

// the admission rules of crtfx_sited.h
bool row_fits(const int32_t* row, const int32_t* off, bool deep) {
    const long long half = 1LL << (SH + WSH - 1), lim = 1LL << 31;
    if (!deep) return (mag(row[0]) + mag(row[1]) + mag(row[2])) * 255 * 16 + half < lim;
    long long span[3];
    for (int i = 0; i < 3; ++i) span[i] = 16LL * (off[i] > 1023 - off[i] ? off[i] : 1023 - off[i]);
    return mag(row[0]) * span[0] < lim && mag(row[1]) * span[1] + mag(row[2]) * span[2] + half < lim;
}

}  // namespace

extern "C" {

const char* crtfx_sited_last_error(const crtfx_sited* p) { return p ? p->err.c_str() : create_err<crtfx_sited>().c_str(); }

int crtfx_sited_create(int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, crtfx_sited** out_plan) {
    using H = crtfx_sited;
    if (const int rc = begin_create(out_plan)) return rc;
    const bool known = layout >= CRTFX_SITED_YUV420P && layout <= CRTFX_SITED_P010LE;
    const bool deep = known && is_deep(layout);
    if (known && pix_fmt == (deep ? CRTFX_PIX_U8 : CRTFX_PIX_F16))
        return fail<H>(nullptr, CRTFX_E_UNSUPPORTED, deep ? "only half RGB frames are written from %s (uint8 frames take an 8-bit layout)"
                                                           : "only uint8 RGB frames are written from %s (half frames take a 10-bit layout)", LAYOUT_NAMES[layout]);
    if (const int rc = check_create<H>(pix_fmt, known ? (deep ? CRTFX_PIX_F16 : CRTFX_PIX_U8) : pix_fmt == CRTFX_PIX_F16 ? CRTFX_PIX_F16 : CRTFX_PIX_U8,
                                       h, w, layout, known, m, off, deep ? 1023 : 255)) return rc;
    if (!row_fits(m, off, deep) || !row_fits(m + 3, off, deep) || !row_fits(m + 6, off, deep))
        return fail<H>(nullptr, CRTFX_E_INVALID, "the matrix lets an accumulator leave int32");
    H* p = nullptr;
    if (const int rc = new_plan(false, device, layout, h, w, m, &p)) return rc;
    Args& a = p->args;
    a.rows = is_420(layout) ? (h + 1) / 2 : h; a.cw = (w + 1) / 2;
    a.k[0] = off[0]; a.k[1] = off[1] << WSH; a.k[2] = off[2] << WSH;
    set_siting(p, CRTFX_SITED_LEFT);
    const size_t luma = (size_t)h * w, chroma = 2 * (size_t)a.rows * a.cw;
    if (layout == CRTFX_SITED_YUYV422 || layout == CRTFX_SITED_UYVY422) p->frame_bytes = 4 * (size_t)h * a.cw;
    else p->frame_bytes = (luma + chroma) * (deep ? 2 : 1);
    p->rgb_bytes = luma * (deep ? 6 : 3);
    Unit::note_plan(p, vec_fits(p, nullptr, 0, nullptr, 0, 1), 0);
    *out_plan = p;
    return CRTFX_OK;
}

int crtfx_sited_destroy(crtfx_sited* p) { return destroy(p); }
size_t crtfx_sited_frame_bytes(const crtfx_sited* p) { return p ? p->frame_bytes : 0; }

int crtfx_sited_set_option(crtfx_sited* p, int option, int value) {
    if (!p || option != CRTFX_SITED_OPT_SITING) return set_option<Unit>(p, option, value);
    if (value != CRTFX_SITED_LEFT && value != CRTFX_SITED_CENTER) return fail(p, CRTFX_E_INVALID, "SITING takes 0 (left) or 1 (center), got %d", value);
    set_siting(p, value);
    Unit::note_plan(p, vec_fits(p, nullptr, 0, nullptr, 0, 1), 0);
    return CRTFX_OK;
}

int crtfx_sited_last_plan(crtfx_sited* p, char* buf, size_t n) { return last_plan(p, buf, n); }
int crtfx_sited_run(crtfx_sited* p, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream) {
    return run_frames<Unit>(p, src_base, src_stride_bytes, dst_base, dst_stride_bytes, n, stream);
}

}  // extern "C"
