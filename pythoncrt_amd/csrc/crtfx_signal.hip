// crtfx_signal.hip — the composite-video stage (include/crtfx_signal.h): every row of an h x w x 3 frame is encoded to an NTSC-like signal
// sampled at four times the colour subcarrier and decoded again, in integers.  A vec and a general kernel per (signal, chroma filter, sample
// type), the host glue, the C entry points.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <type_traits>

#include "crtfx_signal.h"
#include "crtfx_edge.hip.h"
#include "crtfx_frame_host.h"

namespace crtfx_signal_impl {

using namespace crtfx_deint_impl;       // the path tags, u8 / f16 with the quarter-code quantiser, load_dwords / store_dwords, BLOCK

// The two signals and the two decoder chroma filters.  D is the triangle [1 2 .. reach + 1 .. 2 1], which sums to (reach + 1)^2 = 1 << shift.
struct composite { static constexpr const char* name = "composite"; static constexpr bool crosstalk = true; };
struct svideo { static constexpr const char* name = "svideo"; static constexpr bool crosstalk = false; };
struct sharp { static constexpr const char* name = "sharp"; static constexpr int reach = 3, shift = 4; };
struct soft { static constexpr const char* name = "soft"; static constexpr int reach = 7, shift = 6; };

constexpr int ENC = 3;                  // the reach of the encoder's T7
constexpr int NOTCH = 2;                // the reach of the luma notch

// cos and sin of phase p (0..3) as selections: v * cos[p] is cos_of(p, v)
__host__ __device__ constexpr int cos_of(int p, int v) { return p == 0 ? v : p == 2 ? -v : 0; }
__host__ __device__ constexpr int sin_of(int p, int v) { return p == 1 ? v : p == 3 ? -v : 0; }
__host__ __device__ constexpr int tri(int m, int reach) { return m <= reach ? m + 1 : 2 * reach + 1 - m; }      // tap m = 0 .. 2 reach of a triangle

// step 1
__device__ __forceinline__ void to_yiq(int r, int g, int b, int& y, int& i, int& q) {
    y = (1225 * r + 2404 * g + 467 * b + 128) >> 8;
    i = (2441 * r - 1125 * g - 1316 * b + 128) >> 8;
    q = (866 * r - 2141 * g + 1275 * b + 128) >> 8;
}

// step 7, clamped to 0..M.  The accumulator is clamped to 0 .. (M << 16) + 65535 and then shifted, which is the shift clamped to 0..M (a
// floor is monotone).  In the other order the compiler fuses two bytes' shift and clamp into v_ashr_pk_u8_i32 and ORs further bytes into the
// upper half of its result, which it takes to be zero; on the MI355X the u8 vec builds then wrote byte 2 of every dword OR'ed with the low
// byte of that dword's first accumulator >> 16 — what the instruction's destination, which was its first operand, held before
template <int M>
__device__ __forceinline__ void to_rgb(int yd, int id, int qd, int (&c)[3]) {
    constexpr int TOP = (M << 16) | 0xffff;
    c[0] = 4096 * yd + 3916 * id + 2543 * qd + 32768;
    c[1] = 4096 * yd - 1114 * id - 2651 * qd + 32768;
    c[2] = 4096 * yd - 4533 * id + 6981 * qd + 32768;
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = (c[k] < 0 ? 0 : (c[k] > TOP ? TOP : c[k])) >> 16;
}

// Launch constants.
struct Args {
    const uint8_t* src;
    uint8_t* dst;
    size_t src_stride, dst_stride;      // bytes
    uint32_t h, w;
    uint32_t nseg;                      // vec: segments per row
    uint32_t units;                     // vec: segments per frame (h * nseg)
    uint32_t t0;                        // the parity of t of this launch's first frame, 0 without crawl
    uint32_t crawl;
};

// ---- vec: one wave per segment of SEG pixels of one row; the cascade is staged through the wave's own int16 planes in LDS ----

constexpr int SEG = 488;                // pixels of a segment: with the widest halo (12 to either side) 512 = 64 lanes x 8
constexpr int PLANE = 528;              // int16 entries of a plane: the 512 staged and what the widest read behind them touches
constexpr int WAVES = BLOCK / 64;
typedef short short8 __attribute__((ext_vector_type(8)));
typedef short short4 __attribute__((ext_vector_type(4)));

template <class S, class C, class P>
__device__ __forceinline__ void signal_vec(const Args& a) {
    constexpr int SZ = sizeof(typename P::T), R = C::reach, H = R + NOTCH + ENC, GD = 3 * SZ;       // GD: dwords of four pixels
    constexpr int M = SZ == 1 ? 255 : 1020;
    static_assert(SEG % 8 == 0 && H % 4 == 0 && SEG + 2 * H <= 512, "a segment and its halo are 64 lanes x 8 pixels");
    __shared__ __attribute__((aligned(16))) short lds[WAVES][4][PLANE];         // per wave: Y0, I0, Q0, and s (C under svideo)
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t u = blockIdx.x * WAVES + wave;
    const bool live = u < a.units;
    const uint32_t uu = live ? u : a.units - 1u;                                // a wave past the end repeats the last unit and stores nothing
    const uint32_t y = uu / a.nseg, sx = uu - y * a.nseg;
    const int w = (int)a.w, x0 = (int)sx * SEG, segw = w - x0 < SEG ? w - x0 : SEG;
    const size_t row = (size_t)a.w * 3u * SZ;
    const uint8_t* __restrict__ s = a.src + (size_t)blockIdx.z * a.src_stride + (size_t)y * row;
    short (*pl)[PLANE] = lds[wave];
    const bool flip = ((y + (a.crawl ? a.t0 + blockIdx.z : 0u)) & 1u) != 0u;    // 180 degrees per line and per frame
    const int l8 = 8 * (int)lane;

    // steps 1: plane index p is pixel x0 - H + p; the lane stages p = 8 lane .. 8 lane + 7 as two groups of four pixels.  A group lies inside
    // the row or outside it (w % 8 == 0, x0 % 8 == 0, H % 4 == 0); one outside is the edge pixel of the group at the edge
    if (l8 < segw + 2 * H) {
        short8 yv, iv, qv;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int gs = x0 - H + l8 + 4 * g;
            const int gc = gs < 0 ? 0 : (gs >= w ? w - 4 : gs);
            uint32_t wd[GD];
            load_dwords<GD>(s + (size_t)gc * 3u * SZ, wd);
            int q[12];
            unpack_codes<P, GD>(wd, q);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int c[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) c[k] = gs < 0 ? q[k] : (gs >= w ? q[9 + k] : q[3 * i + k]);
                int yy, ii, qq;
                to_yiq(c[0], c[1], c[2], yy, ii, qq);
                yv[4 * g + i] = (short)yy; iv[4 * g + i] = (short)ii; qv[4 * g + i] = (short)qq;
            }
        }
        *reinterpret_cast<short8*>(&pl[0][l8]) = yv;
        *reinterpret_cast<short8*>(&pl[1][l8]) = iv;
        *reinterpret_cast<short8*>(&pl[2][l8]) = qv;
    }
    __syncthreads();

    // steps 2 - 4: s index j is pixel x0 - R - NOTCH + j = plane index j + ENC; the lane forms j = 8 lane .. 8 lane + 7 from plane entries
    // 8 lane .. 8 lane + 13.  x0 % 4 == 0, so the phase of entry i is a constant of i, turned by 180 degrees where flip
    {
        short8 t[3][2];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            t[k][0] = *reinterpret_cast<const short8*>(&pl[k][l8]);
            t[k][1] = *reinterpret_cast<const short8*>(&pl[k][l8 + 8]);
        }
        short8 sv;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            constexpr int OFF = 64 - R - NOTCH;                                 // = -(R + NOTCH) mod 4
            const int ph = (i + OFF) & 3;
            const int plane = (ph & 1) ? 2 : 1;                                 // sin: Q1, cos: I1 — the other product is zero
            int acc = 8;
#pragma unroll
            for (int k = 0; k <= 2 * ENC; ++k) acc += tri(k, ENC) * (int)t[plane][(i + k) >> 3][(i + k) & 7];
            const int v = acc >> 4;
            int c = (ph & 1) ? sin_of(ph, v) : cos_of(ph, v);
            c = flip ? -c : c;
            sv[i] = (short)((S::crosstalk ? (int)t[0][(i + ENC) >> 3][(i + ENC) & 7] : 0) + c);
        }
        *reinterpret_cast<short8*>(&pl[3][l8]) = sv;
    }
    __syncthreads();

    // steps 4 - 7: the lane owns pixels x0 + 8 lane .. + 7; e index i is pixel x0 + 8 lane + i - R = s index 8 lane + i + NOTCH
    if (!live || l8 >= segw) return;
    constexpr int NE = 8 + 2 * R, NS = NE + 2 * NOTCH, NV = (NS + 7) / 8;
    short8 sq[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) sq[k] = *reinterpret_cast<const short8*>(&pl[3][l8 + 8 * k]);
    int e[NE], d[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        const int c = (int)sq[(i + 2) >> 3][(i + 2) & 7];
        if constexpr (S::crosstalk) {
            const int lo = (int)sq[i >> 3][i & 7], hi = (int)sq[(i + 4) >> 3][(i + 4) & 7];
            e[i] = c - ((lo + 2 * c + hi + 2) >> 2);
        } else {
            e[i] = c;
        }
        constexpr int OFF = 64 - R;
        const int ph = (i + OFF) & 3;
        const int v = (ph & 1) ? sin_of(ph, 2 * e[i]) : cos_of(ph, 2 * e[i]);   // odd phases carry Qd0, even ones Id0
        d[i] = flip ? -v : v;
    }
    short yq[8];
    if constexpr (!S::crosstalk) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const short4 t = *reinterpret_cast<const short4*>(&pl[0][l8 + H + 4 * g]);
#pragma unroll
            for (int i = 0; i < 4; ++i) yq[4 * g + i] = t[i];
        }
    }
    int out[24];
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        constexpr int OFF = 64 - R;
        int ai = 1 << (C::shift - 1), aq = ai;
#pragma unroll
        for (int m = 0; m <= 2 * R; ++m) {
            if (((o + m + OFF) & 1) == 0) ai += tri(m, R) * d[o + m]; else aq += tri(m, R) * d[o + m];
        }
        int yd;
        if constexpr (S::crosstalk) yd = (int)sq[(o + R + 2) >> 3][(o + R + 2) & 7] - e[o + R]; else yd = (int)yq[o];
        int c[3];
        to_rgb<M>(yd, ai >> C::shift, aq >> C::shift, c);
#pragma unroll
        for (int k = 0; k < 3; ++k) out[3 * o + k] = c[k];
    }
    constexpr int SPD = P::SPD, OD = 24 / SPD;
    uint32_t od[OD];
#pragma unroll
    for (int j = 0; j < OD; ++j) {
        uint32_t v = 0u;
#pragma unroll
        for (int t = 0; t < SPD; ++t) v |= P::bits(out[j * SPD + t]) << (8 * SZ * t);
        od[j] = v;
    }
    store_dwords<OD>(a.dst + (size_t)blockIdx.z * a.dst_stride + (size_t)y * row + (size_t)(x0 + l8) * 3u * SZ, od);
}

// ---- general: one lane per pixel; the cascade of that pixel from clamped loads ----

template <class S, class C, class P>
__device__ __forceinline__ void signal_general(const Args& a) {
    typedef typename P::T T;
    constexpr int R = C::reach, H = R + NOTCH + ENC, NW = 2 * H + 1, NS = 2 * (R + NOTCH) + 1, NE = 2 * R + 1;
    constexpr int M = sizeof(T) == 1 ? 255 : 1020;
    const int x = (int)(blockIdx.x * BLOCK + threadIdx.x), w = (int)a.w;
    const uint32_t y = blockIdx.y;
    if (x >= w) return;
    const size_t row = (size_t)a.w * 3u;
    const T* __restrict__ s = reinterpret_cast<const T*>(a.src + (size_t)blockIdx.z * a.src_stride) + (size_t)y * row;
    const int turn = (int)(((y + (a.crawl ? a.t0 + blockIdx.z : 0u)) & 1u) * 2u);
    int y0[NW], i0[NW], q0[NW];                                                 // entry p: pixel x - H + p
#pragma unroll
    for (int p = 0; p < NW; ++p) {
        const int xx = x - H + p, xc = xx < 0 ? 0 : (xx >= w ? w - 1 : xx);
        const T* px = s + (size_t)xc * 3u;
        to_yiq(P::code(px[0]), P::code(px[1]), P::code(px[2]), y0[p], i0[p], q0[p]);
    }
    int sg[NS];                                                                 // entry j: pixel x - R - NOTCH + j
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        int ai = 8, aq = 8;
#pragma unroll
        for (int k = 0; k <= 2 * ENC; ++k) { ai += tri(k, ENC) * i0[j + k]; aq += tri(k, ENC) * q0[j + k]; }
        const int ph = (x - R - NOTCH + j + turn) & 3;
        const int c = cos_of(ph, ai >> 4) + sin_of(ph, aq >> 4);
        sg[j] = (S::crosstalk ? y0[j + ENC] : 0) + c;
    }
    int ai = 1 << (C::shift - 1), aq = ai;
#pragma unroll
    for (int i = 0; i < NE; ++i) {                                              // entry i: pixel x - R + i
        const int c = sg[i + NOTCH];
        const int e = S::crosstalk ? c - ((sg[i] + 2 * c + sg[i + 2 * NOTCH] + 2) >> 2) : c;
        const int ph = (x - R + i + turn) & 3;
        ai += tri(i, R) * cos_of(ph, 2 * e);
        aq += tri(i, R) * sin_of(ph, 2 * e);
    }
    const int yd = S::crosstalk ? (sg[R] + 2 * sg[R + NOTCH] + sg[R + 2 * NOTCH] + 2) >> 2 : y0[H];
    int c[3];
    to_rgb<M>(yd, ai >> C::shift, aq >> C::shift, c);
    T* __restrict__ d = reinterpret_cast<T*>(a.dst + (size_t)blockIdx.z * a.dst_stride) + (size_t)y * row + (size_t)x * 3u;
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = (T)P::bits(c[k]);
}

template <class S, class C, class P, class Path>
__global__ __launch_bounds__(BLOCK) void k_signal(Args a) {
    if constexpr (std::is_same<Path, vec>::value) signal_vec<S, C, P>(a); else signal_general<S, C, P>(a);
}

}  // namespace crtfx_signal_impl

using namespace crtfx_signal_impl;

struct crtfx_signal : crtfx_frames::Plan {     // one frame size and sample type on both sides
    int h = 0, w = 0;
    bool half = false, svid = false, wide = false, crawl = false;
    int64_t first_index = 0;                    // of the run under way: crtfx_signal_run carries it into launch
};

namespace {

using crtfx_frames::Batch;
using crtfx_stage::create_err;
using crtfx_stage::fail;

template <class S, class C, class P>
void launch_path(bool fits, dim3 grid, hipStream_t st, const Args& a) {
    if (fits) hipLaunchKernelGGL((k_signal<S, C, P, vec>), grid, dim3(BLOCK), 0, st, a);
    else hipLaunchKernelGGL((k_signal<S, C, P, general>), grid, dim3(BLOCK), 0, st, a);
}

template <class S, class C>
void launch_pix(const crtfx_signal* p, bool fits, dim3 grid, hipStream_t st, const Args& a) {
    if (p->half) launch_path<S, C, f16>(fits, grid, st, a); else launch_path<S, C, u8>(fits, grid, st, a);
}

template <class S>
void launch_chroma(const crtfx_signal* p, bool fits, dim3 grid, hipStream_t st, const Args& a) {
    if (p->wide) launch_pix<S, soft>(p, fits, grid, st, a); else launch_pix<S, sharp>(p, fits, grid, st, a);
}

struct U : crtfx_frames::Unit {
    using H = crtfx_signal;
    static constexpr int force_option = CRTFX_SIGNAL_OPT_FORCE_GENERAL;
    static constexpr const char* name = "signal";
    static constexpr bool one_size = true;

    // the vec kernels' conditions (crtfx_signal.h)
    static bool vec_fits(const H* p, const Batch& b) {
        if (p->force_general || (p->w & 7)) return false;
        if ((reinterpret_cast<uintptr_t>(b.src) | reinterpret_cast<uintptr_t>(b.dst)) & 3u) return false;
        return b.n <= 1 || !((b.src_stride | b.dst_stride) & 3u);
    }

    static void note_plan(H* p, bool fits, int frames) {
        snprintf(p->plan, sizeof p->plan, "signal=k_signal<%s,%s,%s,%s>;frames=%d", p->svid ? svideo::name : composite::name,
                 p->wide ? soft::name : sharp::name, p->half ? f16::name : u8::name, fits ? vec::name : general::name, frames);
    }

    static Args make_args(const H* p, bool, const Batch&) {
        Args a{};
        a.h = (uint32_t)p->h; a.w = (uint32_t)p->w;
        a.nseg = (a.w + SEG - 1) / SEG;
        a.units = a.h * a.nseg;                                         // below 2^22
        a.crawl = p->crawl ? 1u : 0u;
        return a;
    }

    static void launch(const H* p, bool fits, Args& a, int f, unsigned g, hipStream_t st) {
        a.t0 = (uint32_t)((p->first_index + f) & 1);
        const dim3 grid = fits ? dim3((a.units + WAVES - 1) / WAVES, 1, g) : dim3((a.w + BLOCK - 1) / BLOCK, p->h, g);
        if (p->svid) launch_chroma<svideo>(p, fits, grid, st, a); else launch_chroma<composite>(p, fits, grid, st, a);
    }
};

}  // namespace

extern "C" {

const char* crtfx_signal_last_error(const crtfx_signal* p) { return p ? p->err.c_str() : create_err<crtfx_signal>().c_str(); }

int crtfx_signal_create(int device, int h, int w, int pix_fmt, int signal, int chroma, int crawl, crtfx_signal** out_plan) {
    using H = crtfx_signal;
    if (const int rc = crtfx_frames::begin_create(out_plan)) return rc;
    if (const int rc = crtfx_frames::check_size<H>("h", h)) return rc;
    if (const int rc = crtfx_frames::check_size<H>("w", w)) return rc;
    if (pix_fmt != CRTFX_PIX_U8 && pix_fmt != CRTFX_PIX_F16) return fail<H>(nullptr, CRTFX_E_INVALID, "unknown pix_fmt %d", pix_fmt);
    if (signal != CRTFX_SIGNAL_COMPOSITE && signal != CRTFX_SIGNAL_SVIDEO) return fail<H>(nullptr, CRTFX_E_INVALID, "unknown signal %d", signal);
    if (chroma != CRTFX_SIGNAL_SHARP && chroma != CRTFX_SIGNAL_SOFT) return fail<H>(nullptr, CRTFX_E_INVALID, "unknown chroma %d", chroma);
    if (crawl != 0 && crawl != 1) return fail<H>(nullptr, CRTFX_E_INVALID, "crawl = %d is neither 0 nor 1", crawl);
    return crtfx_frames::new_plan<U>(device, out_plan, [&](H* p) {
        p->h = h; p->w = w;
        p->half = pix_fmt == CRTFX_PIX_F16; p->svid = signal == CRTFX_SIGNAL_SVIDEO; p->wide = chroma == CRTFX_SIGNAL_SOFT; p->crawl = crawl != 0;
        p->src_bps = p->dst_bps = p->half ? 2 : 1;
        p->src_bytes = p->dst_bytes = (size_t)h * w * 3 * p->src_bps;
        return CRTFX_OK;
    });
}

int crtfx_signal_destroy(crtfx_signal* p) { return crtfx_frames::destroy(p); }

int crtfx_signal_set_option(crtfx_signal* p, int option, int value) { return crtfx_frames::set_option<U>(p, option, value); }

int crtfx_signal_last_plan(crtfx_signal* p, char* buf, size_t n) { return crtfx_frames::last_plan(p, buf, n); }

int crtfx_signal_run(crtfx_signal* p, int64_t first_index, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n,
                     void* stream) {
    if (!p) return CRTFX_E_INVALID;
    if (first_index < 0) return fail(p, CRTFX_E_INVALID, "first_index = %lld is negative", (long long)first_index);
    p->first_index = first_index;
    return crtfx_frames::run<U>(p, Batch{nullptr, src_base, src_stride_bytes, dst_base, dst_stride_bytes, n}, stream);
}

}  // extern "C"
