// crtfx_egress_sited.hip — the sited egress stage of libcrtfx.so (include/crtfx_egress_sited.h): finished RGB frames -> the seven sub-sampled
// layouts of crtfx_egress_*, crtfx_egress422_* and crtfx_egress10_* with chroma FILTERED onto a stated siting instead of box-averaged.  A
// translation unit of its own: it shares no kernel, table or handle with the effect chain or the other stages.  The host code around the
// kernels (checks, frame-group loop, error strings) is the skeleton of crtfx_stage_host.h; the siting option is this unit's own.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <type_traits>

#include "crtfx_egress_sited.h"
#include "crtfx_stage_host.h"

namespace crtfx_egress_sited_impl {

constexpr int BLOCK = 256;
constexpr int SH = 16;                          // fractional bits of the matrix; the chroma sums (weights in quarters) carry two or three more
constexpr int GENERAL = 0, VEC = 1;             // the PATH template argument; LAYOUT is a crtfx_sited_layout

struct Args {
    const uint8_t* src; size_t src_stride;
    uint8_t* dst; size_t dst_stride;
    int h, w, rows, cw;                         // rows: chroma rows, (h + 1) / 2 for 4:2:0 and h for 4:2:2
    int m[9];                                   // rows Y, U, V over the columns R, G, B
    int k[3];                                   // (off0 << SH) + half for Y; (off << CSH) + half for U, V
    int wt[3];                                  // the horizontal weights of the pixel left of, on and right of column 2 cx: the siting
};

// unsigned dwords at 4-byte alignment: the widest access the vec path's rule (crtfx_egress_sited.h) guarantees
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
    static constexpr int CSH = SH + (v420 ? 3 : 2);            // the shift of a chroma sum: weights sum to 8 (4:2:0) or 4 (4:2:2)
    // byte positions inside a packed macropixel: yuyv422 = Y0 U Y1 V, uyvy422 = U Y0 V Y1
    static constexpr int Y0 = LAYOUT == CRTFX_SITED_YUYV422 ? 0 : 1, Y1 = Y0 + 2, U = LAYOUT == CRTFX_SITED_YUYV422 ? 1 : 0, V = U + 2;
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

// create admits only matrices whose accumulators stay in [0, 2^31): the lower clamp can never act, the shift is a logical one and the upper
// clamp is an unsigned minimum (the form of crtfx_egress.hip, for the reason given there).
template <int LAYOUT> __device__ __forceinline__ unsigned luma(const Args& a, const int (&p)[3]) {
    return min((unsigned)(a.m[0] * p[0] + a.m[1] * p[1] + a.m[2] * p[2] + a.k[0]) >> SH, Traits<LAYOUT>::top);
}
template <int LAYOUT> __device__ __forceinline__ unsigned chroma(const Args& a, int row, const int (&s)[3]) {
    return min((unsigned)(a.m[3 * row] * s[0] + a.m[3 * row + 1] * s[1] + a.m[3 * row + 2] * s[2] + a.k[row]) >> Traits<LAYOUT>::CSH, Traits<LAYOUT>::top);
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

// vec (w % 8 == 0, 4-byte-aligned frame bases): one lane = 8 columns of one (4:2:2) or two (4:2:0) rows; consecutive lanes, consecutive
// column blocks.  The pixel left of the block is read with one narrow load per row at a clamped index.
// general: one lane = one chroma sample and the (up to) 2 x 2 or 2 x 1 luma samples under it; bytes (8-bit) or 16-bit words (10-bit) only.
template <int LAYOUT, int PATH>
__global__ __launch_bounds__(BLOCK) void k_egress_sited(Args a) {
    using T = Traits<LAYOUT>;
    const uint8_t* fsrc = a.src + (size_t)blockIdx.z * a.src_stride;
    uint8_t* fdst = a.dst + (size_t)blockIdx.z * a.dst_stride;
    const int idx = blockIdx.x * BLOCK + threadIdx.x;
    const int per_row = PATH == VEC ? a.w >> 3 : a.cw;
    if (idx >= a.rows * per_row) return;
    const int cy = idx / per_row, bx = idx - cy * per_row;     // general: bx is the chroma column
    const int y0 = T::v420 ? 2 * cy : cy;
    const bool below = T::v420 && y0 + 1 < a.h;
    const int yy[2] = {y0, below ? y0 + 1 : y0};
    const size_t E = T::deep ? 2 : 1;                          // bytes of a sample
    if (PATH == VEC) {
        typename T::Row blk[T::NR];
        int prev[T::NR][3];                                    // the pixel left of the one in hand; first the one left of the block
        const int xl = max(8 * bx - 1, 0);
#pragma unroll
        for (int r = 0; r < T::NR; ++r) {
            blk[r] = *reinterpret_cast<const typename T::Row*>(fsrc + ((size_t)yy[r] * a.w + (size_t)bx * 8) * 3 * E);
            pixel_at<LAYOUT>(fsrc, a, yy[r], xl, prev[r]);
        }
        unsigned yq[T::NR][8], uq[4], vq[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {           // chroma sample q = columns 2q (where "left" sits), 2q + 1
            int s[3] = {0, 0, 0};
#pragma unroll
            for (int r = 0; r < T::NR; ++r) {
                int own[3], right[3];
                pixel_of<LAYOUT>(blk[r], 2 * q, own);
                pixel_of<LAYOUT>(blk[r], 2 * q + 1, right);
                yq[r][2 * q] = luma<LAYOUT>(a, own);
                yq[r][2 * q + 1] = luma<LAYOUT>(a, right);
#pragma unroll
                for (int c = 0; c < 3; ++c) { s[c] += a.wt[0] * prev[r][c] + a.wt[1] * own[c] + a.wt[2] * right[c]; prev[r][c] = right[c]; }
            }
            uq[q] = chroma<LAYOUT>(a, 1, s);
            vq[q] = chroma<LAYOUT>(a, 2, s);
        }
        // ---- stores: the dword-multiple accesses of the layout's box kernel ----
        if (T::packed) {
            U4 mp;
#pragma unroll
            for (int q = 0; q < 4; ++q) mp.v[q] = (yq[0][2 * q] << (8 * T::Y0)) | (yq[0][2 * q + 1] << (8 * T::Y1)) | (uq[q] << (8 * T::U)) | (vq[q] << (8 * T::V));
            *reinterpret_cast<U4*>(fdst + (size_t)y0 * a.w * 2 + (size_t)bx * 16) = mp;
            return;
        }
#pragma unroll
        for (int r = 0; r < T::NR; ++r) {
            if (r == 1 && !below) break;
            if (T::deep) {
                U4 o;
#pragma unroll
                for (int i = 0; i < 4; ++i) o.v[i] = word<LAYOUT>(yq[r][2 * i]) | (word<LAYOUT>(yq[r][2 * i + 1]) << 16);
                *reinterpret_cast<U4*>(fdst + ((size_t)(y0 + r) * a.w + (size_t)bx * 8) * 2) = o;
            } else {
                U2 o;
#pragma unroll
                for (int i = 0; i < 2; ++i) o.v[i] = yq[r][4 * i] | (yq[r][4 * i + 1] << 8) | (yq[r][4 * i + 2] << 16) | (yq[r][4 * i + 3] << 24);
                *reinterpret_cast<U2*>(fdst + (size_t)(y0 + r) * a.w + (size_t)bx * 8) = o;
            }
        }
        uint8_t* cbase = fdst + (size_t)a.h * a.w * E;
        const size_t plane = (size_t)a.rows * a.cw * E;
        if (T::deep && T::semi) {               // u0 v0 | u1 v1 | u2 v2 | u3 v3
            U4 uv;
#pragma unroll
            for (int q = 0; q < 4; ++q) uv.v[q] = word<LAYOUT>(uq[q]) | (word<LAYOUT>(vq[q]) << 16);
            *reinterpret_cast<U4*>(cbase + (size_t)cy * a.w * 2 + (size_t)bx * 16) = uv;
        } else if (T::deep) {
            const size_t o = ((size_t)cy * a.cw + (size_t)bx * 4) * 2;
            U2 up, vp;
#pragma unroll
            for (int i = 0; i < 2; ++i) { up.v[i] = word<LAYOUT>(uq[2 * i]) | (word<LAYOUT>(uq[2 * i + 1]) << 16); vp.v[i] = word<LAYOUT>(vq[2 * i]) | (word<LAYOUT>(vq[2 * i + 1]) << 16); }
            *reinterpret_cast<U2*>(cbase + o) = up;
            *reinterpret_cast<U2*>(cbase + plane + o) = vp;
        } else if (T::semi) {                   // u0 v0 u1 v1 | u2 v2 u3 v3
            U2 uv;
#pragma unroll
            for (int i = 0; i < 2; ++i) uv.v[i] = uq[2 * i] | (vq[2 * i] << 8) | (uq[2 * i + 1] << 16) | (vq[2 * i + 1] << 24);
            *reinterpret_cast<U2*>(cbase + (size_t)cy * a.w + (size_t)bx * 8) = uv;
        } else {
            const size_t o = (size_t)cy * a.cw + (size_t)bx * 4;
            *reinterpret_cast<unsigned*>(cbase + o) = uq[0] | (uq[1] << 8) | (uq[2] << 16) | (uq[3] << 24);
            *reinterpret_cast<unsigned*>(cbase + plane + o) = vq[0] | (vq[1] << 8) | (vq[2] << 16) | (vq[3] << 24);
        }
    } else {
        const int x0 = 2 * bx;
        const bool right = x0 + 1 < a.w;
        const int xl = max(x0 - 1, 0), xr = right ? x0 + 1 : x0;
        int s[3] = {0, 0, 0};
        unsigned ya[T::NR], yb[T::NR];
#pragma unroll
        for (int r = 0; r < T::NR; ++r) {
            int pl[3], p0[3], pr[3];
            pixel_at<LAYOUT>(fsrc, a, yy[r], xl, pl);
            pixel_at<LAYOUT>(fsrc, a, yy[r], x0, p0);
            pixel_at<LAYOUT>(fsrc, a, yy[r], xr, pr);
            ya[r] = luma<LAYOUT>(a, p0);
            yb[r] = luma<LAYOUT>(a, pr);        // at an odd edge: the row's last Y again, the pad byte of a packed row
#pragma unroll
            for (int c = 0; c < 3; ++c) s[c] += a.wt[0] * pl[c] + a.wt[1] * p0[c] + a.wt[2] * pr[c];
        }
        const unsigned u = chroma<LAYOUT>(a, 1, s), v = chroma<LAYOUT>(a, 2, s);
        if (T::packed) {
            uint8_t* mp = fdst + ((size_t)y0 * a.cw + bx) * 4;
            mp[T::Y0] = (uint8_t)ya[0]; mp[T::Y1] = (uint8_t)yb[0]; mp[T::U] = (uint8_t)u; mp[T::V] = (uint8_t)v;
            return;
        }
        const size_t o = (size_t)cy * a.cw + bx, plane = (size_t)a.rows * a.cw, luma_n = (size_t)a.h * a.w;
        if (T::deep) {
            uint16_t* f16 = reinterpret_cast<uint16_t*>(fdst);
#pragma unroll
            for (int r = 0; r < T::NR; ++r) {
                if (r == 1 && !below) break;
                uint16_t* y = f16 + (size_t)(y0 + r) * a.w + x0;
                y[0] = (uint16_t)word<LAYOUT>(ya[r]);
                if (right) y[1] = (uint16_t)word<LAYOUT>(yb[r]);
            }
            uint16_t* cb = f16 + luma_n;
            if (T::semi) { cb[2 * o] = (uint16_t)word<LAYOUT>(u); cb[2 * o + 1] = (uint16_t)word<LAYOUT>(v); }
            else { cb[o] = (uint16_t)word<LAYOUT>(u); cb[plane + o] = (uint16_t)word<LAYOUT>(v); }
        } else {
#pragma unroll
            for (int r = 0; r < T::NR; ++r) {
                if (r == 1 && !below) break;
                uint8_t* y = fdst + (size_t)(y0 + r) * a.w + x0;
                y[0] = (uint8_t)ya[r];
                if (right) y[1] = (uint8_t)yb[r];
            }
            uint8_t* cb = fdst + luma_n;
            if (T::semi) { cb[2 * o] = (uint8_t)u; cb[2 * o + 1] = (uint8_t)v; }
            else { cb[o] = (uint8_t)u; cb[plane + o] = (uint8_t)v; }
        }
    }
}

}  // namespace crtfx_egress_sited_impl

using namespace crtfx_egress_sited_impl;
using namespace crtfx_stage;

struct crtfx_egress_sited : StagePlan { Args args{}; int siting = CRTFX_SITED_LEFT; };        // `egress` is always true

namespace {

static_assert(SH == MATRIX_SH, "the matrices are the other egress stages'");

const char* const LAYOUT_NAMES[7] = {"yuv420p", "nv12", "yuv422p", "yuyv422", "uyvy422", "yuv420p10le", "p010le"};
bool is_deep(int layout) { return layout == CRTFX_SITED_YUV420P10LE || layout == CRTFX_SITED_P010LE; }
bool is_420(int layout) { return layout == CRTFX_SITED_YUV420P || layout == CRTFX_SITED_NV12 || is_deep(layout); }

template <int LAYOUT>
void launch_layout(bool vec, dim3 grid, hipStream_t st, const Args& a) {
    if (vec) hipLaunchKernelGGL((k_egress_sited<LAYOUT, VEC>), grid, dim3(BLOCK), 0, st, a);
    else hipLaunchKernelGGL((k_egress_sited<LAYOUT, GENERAL>), grid, dim3(BLOCK), 0, st, a);
}

struct Unit {
    static constexpr int block = BLOCK, force_option = CRTFX_EGRESS_SITED_OPT_FORCE_GENERAL;
    static const char* name(bool) { return "egress_sited"; }
    static void note_plan(crtfx_egress_sited* p, bool vec, int frames) {
        snprintf(p->plan, sizeof p->plan, "egress_sited=k_egress_sited<%s,%s>;siting=%s;frames=%d", LAYOUT_NAMES[p->layout], vec ? "vec" : "general",
                 p->siting == CRTFX_SITED_CENTER ? "center" : "left", frames);
    }
    static int check_alignment(crtfx_egress_sited* p, const void* src_base, size_t src_stride_bytes, const void* dst_base, size_t dst_stride_bytes) {
        if (is_deep(p->layout) && ((reinterpret_cast<uintptr_t>(src_base) | reinterpret_cast<uintptr_t>(dst_base) | src_stride_bytes | dst_stride_bytes) & 1u))
            return fail(p, CRTFX_E_INVALID, "an odd frame base or stride: 16-bit samples need 2-byte alignment");
        return CRTFX_OK;                                                                                  // bytes: any base, any stride
    }
    static int items(const Args& a, bool vec) { return vec ? a.rows * (a.w >> 3) : a.rows * a.cw; }      // at most 32767 * 16384
    static void launch(const crtfx_egress_sited* p, bool vec, dim3 grid, hipStream_t st, const Args& a) {
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

void set_siting(crtfx_egress_sited* p, int siting) {
    Args& a = p->args;
    p->siting = siting;
    if (siting == CRTFX_SITED_CENTER) { a.wt[0] = 0; a.wt[1] = 2; a.wt[2] = 2; }
    else { a.wt[0] = 1; a.wt[1] = 2; a.wt[2] = 1; }
}

}  // namespace

extern "C" {

const char* crtfx_egress_sited_last_error(const crtfx_egress_sited* p) { return p ? p->err.c_str() : create_err<crtfx_egress_sited>().c_str(); }

int crtfx_egress_sited_create(int device, int h, int w, int pix_fmt, int layout, const int32_t* m, const int32_t* off, crtfx_egress_sited** out_plan) {
    using H = crtfx_egress_sited;
    if (const int rc = begin_create(out_plan)) return rc;
    const bool known = layout >= CRTFX_SITED_YUV420P && layout <= CRTFX_SITED_P010LE;
    const bool deep = known && is_deep(layout);
    if (known && pix_fmt == (deep ? CRTFX_PIX_U8 : CRTFX_PIX_F16))
        return fail<H>(nullptr, CRTFX_E_UNSUPPORTED, deep ? "only half RGB frames are converted to %s (uint8 frames take an 8-bit layout)"
                                                           : "only uint8 RGB frames are converted to %s (half frames take a 10-bit layout)", LAYOUT_NAMES[layout]);
    if (const int rc = check_create<H>(pix_fmt, known ? (deep ? CRTFX_PIX_F16 : CRTFX_PIX_U8) : pix_fmt == CRTFX_PIX_F16 ? CRTFX_PIX_F16 : CRTFX_PIX_U8,
                                       h, w, layout, known, m, off, deep ? 1023 : 255)) return rc;
    // the admission rules of crtfx_egress_sited.h: X is the largest weighted sum of per-pixel codes
    const int csh = SH + (is_420(layout) ? 3 : 2);
    const long long top = deep ? 1020 : 255, x = (is_420(layout) ? 8 : 4) * top;
    const long long k[3] = {((long long)off[0] << SH) + (1LL << (SH - 1)), ((long long)off[1] << csh) + (1LL << (csh - 1)), ((long long)off[2] << csh) + (1LL << (csh - 1))};
    if (!egress_row_fits(m, k[0], top) || !egress_row_fits(m + 3, k[1], x) || !egress_row_fits(m + 6, k[2], x))
        return fail<H>(nullptr, CRTFX_E_INVALID, "the matrix lets an accumulator leave [0, 2^31)");
    H* p = nullptr;
    if (const int rc = new_plan(true, device, layout, h, w, m, &p)) return rc;
    Args& a = p->args;
    a.rows = is_420(layout) ? (h + 1) / 2 : h; a.cw = (w + 1) / 2;
    for (int i = 0; i < 3; ++i) a.k[i] = (int)k[i];
    set_siting(p, CRTFX_SITED_LEFT);
    const size_t luma_n = (size_t)h * w, chroma_n = 2 * (size_t)a.rows * a.cw;
    if (layout == CRTFX_SITED_YUYV422 || layout == CRTFX_SITED_UYVY422) p->frame_bytes = 4 * (size_t)h * a.cw;
    else p->frame_bytes = (luma_n + chroma_n) * (deep ? 2 : 1);
    p->rgb_bytes = luma_n * (deep ? 6 : 3);
    Unit::note_plan(p, vec_fits(p, nullptr, 0, nullptr, 0, 1), 0);
    *out_plan = p;
    return CRTFX_OK;
}

int crtfx_egress_sited_destroy(crtfx_egress_sited* p) { return destroy(p); }
size_t crtfx_egress_sited_frame_bytes(const crtfx_egress_sited* p) { return p ? p->frame_bytes : 0; }

int crtfx_egress_sited_set_option(crtfx_egress_sited* p, int option, int value) {
    if (!p || option != CRTFX_EGRESS_SITED_OPT_SITING) return set_option<Unit>(p, option, value);
    if (value != CRTFX_SITED_LEFT && value != CRTFX_SITED_CENTER) return fail(p, CRTFX_E_INVALID, "SITING takes 0 (left) or 1 (center), got %d", value);
    set_siting(p, value);
    Unit::note_plan(p, vec_fits(p, nullptr, 0, nullptr, 0, 1), 0);
    return CRTFX_OK;
}

int crtfx_egress_sited_last_plan(crtfx_egress_sited* p, char* buf, size_t n) { return last_plan(p, buf, n); }
int crtfx_egress_sited_run(crtfx_egress_sited* p, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream) {
    return run_frames<Unit>(p, src_base, src_stride_bytes, dst_base, dst_stride_bytes, n, stream);
}

}  // extern "C"
