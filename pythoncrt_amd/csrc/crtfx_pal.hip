// crtfx_pal.hip — the PAL composite-video stage (include/crtfx_pal.h): every row of an h x w x 3 frame is encoded to a PAL-like signal sampled
// at four times the colour subcarrier and decoded again, in integers, by a decoder with a phase error and — under DELAY — a one-line delay
// line.  A vec and a general kernel per (signal, chroma filter, decoder, sample type), the host glue, the C entry points.  The row cascade
// is staged as crtfx_signal.hip stages its own; what is new is the carrier (270 degrees per line and frame, the V switch), the rotation by
// the phase error and the line of state a wave carries down its strip of rows.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <type_traits>

#include "crtfx_pal.h"
#include "crtfx_edge.hip.h"
#include "crtfx_frame_host.h"

#ifndef CRTFX_PAL_STRIP
#define CRTFX_PAL_STRIP 8               // rows of a vec wave's strip (crtfx_pal.h: chosen by measurement among 8, 16 and 32)
#endif

namespace crtfx_pal_impl {

using namespace crtfx_deint_impl;       // the path tags, u8 / f16 with the quarter-code quantiser, load_dwords / store_dwords, BLOCK

// The two signals, the two decoder chroma filters and the two decoders.  D is the triangle [1 2 .. reach + 1 .. 2 1], which sums to
// (reach + 1)^2 = 1 << shift.
struct composite { static constexpr const char* name = "composite"; static constexpr bool crosstalk = true; };
struct svideo { static constexpr const char* name = "svideo"; static constexpr bool crosstalk = false; };
struct sharp { static constexpr const char* name = "sharp"; static constexpr int reach = 3, shift = 4; };
struct soft { static constexpr const char* name = "soft"; static constexpr int reach = 7, shift = 6; };
struct delay { static constexpr const char* name = "delay"; static constexpr bool line = true; };
struct simple { static constexpr const char* name = "simple"; static constexpr bool line = false; };

constexpr int ENC = 3;                  // the reach of the encoder's T7
constexpr int NOTCH = 2;                // the reach of the luma notch
constexpr int STRIP = CRTFX_PAL_STRIP;

__host__ __device__ constexpr int tri(int m, int reach) { return m <= reach ? m + 1 : 2 * reach + 1 - m; }      // tap m = 0 .. 2 reach of a triangle

// The carrier of one row of one frame: L = y + c t.  Phase p = (x + 3 L) mod 4; at an odd p the sample carries U with the factor sin[p], at an
// even p it carries V with the factor v cos[p], v = +1 where L is even and -1 otherwise.  The other product is zero.
struct Carrier {
    int rot;                            // 3 L mod 4
    int v;
    __device__ __forceinline__ explicit Carrier(uint32_t L) : rot((int)((3u * L) & 3u)), v((L & 1u) ? -1 : 1) {}
    __device__ __forceinline__ bool odd(int x) const { return ((x + rot) & 1) != 0; }
    // the factor of the product that the phase of x keeps: +1 or -1
    __device__ __forceinline__ int factor(int x) const {
        const int p = (x + rot) & 3;
        return p == 1 ? 1 : p == 3 ? -1 : p == 0 ? v : -v;
    }
};

// step 1
__device__ __forceinline__ void to_yuv(int r, int g, int b, int& y, int& u, int& v) {
    y = (1225 * r + 2404 * g + 467 * b + 128) >> 8;
    u = (-603 * r - 1183 * g + 1786 * b + 128) >> 8;
    v = (2518 * r - 2109 * g - 409 * b + 128) >> 8;
}

// step 7: the decoder's phase error, a rotation of (Ud, Vd) by -theta on the switched axes.  vs is v s_theta
__device__ __forceinline__ void rotate(int ud, int vd, int ct, int vs, int& ur, int& vr) {
    ur = (ct * ud + vs * vd + 2048) >> 12;
    vr = (ct * vd - vs * ud + 2048) >> 12;
}

// step 9, clamped to 0..M.  The accumulator is clamped to 0 .. (M << 16) + 65535 and then shifted, which is the shift clamped to 0..M (a
// floor is monotone).  The clamp stays in front of the shift: in the other order the uint8 vec builds of k_signal wrote wrong bytes
// (crtfx_signal.hip)
template <int M>
__device__ __forceinline__ void to_rgb(int yd, int u, int v, int (&c)[3]) {
    constexpr int TOP = (M << 16) | 0xffff;
    c[0] = 4096 * yd + 4670 * v + 32768;
    c[1] = 4096 * yd - 1617 * u - 2379 * v + 32768;
    c[2] = 4096 * yd + 8325 * u + 32768;
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
    uint32_t units;                     // vec: strips of segments per frame (ceil(h / STRIP) * nseg)
    uint32_t t0;                        // t mod 4 of this launch's first frame
    uint32_t crawl;
    int ct, st;                         // llrint(4096 cos theta), llrint(4096 sin theta)
};

// ---- vec: one wave per segment of SEG pixels and strip of STRIP rows; a row's cascade is staged through the wave's own int16 planes in LDS,
// and the previous row's Ur / Vr of the lane's eight pixels stay in registers: the delay line ----

constexpr int SEG = 488;                // pixels of a segment: with the widest halo (12 to either side) 512 = 64 lanes x 8
constexpr int PLANE = 528;              // int16 entries of a plane: the 512 staged and what the widest read behind them touches
constexpr int WAVES = BLOCK / 64;
typedef short short8 __attribute__((ext_vector_type(8)));
typedef short short4 __attribute__((ext_vector_type(4)));

template <class S, class C, class Dec, class P>
__device__ __forceinline__ void pal_vec(const Args& a) {
    constexpr int SZ = sizeof(typename P::T), R = C::reach, H = R + NOTCH + ENC, GD = 3 * SZ;       // GD: dwords of four pixels
    constexpr int M = SZ == 1 ? 255 : 1020;
    static_assert(SEG % 8 == 0 && H % 4 == 0 && SEG + 2 * H <= 512, "a segment and its halo are 64 lanes x 8 pixels");
    __shared__ __attribute__((aligned(16))) short lds[WAVES][4][PLANE];         // per wave: Y0, U0, V0, and s (C under svideo)
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t u = blockIdx.x * WAVES + wave;
    const bool live = u < a.units;
    const uint32_t uu = live ? u : a.units - 1u;                                // a wave past the end repeats the last unit and stores nothing
    const uint32_t strip = uu / a.nseg, sx = uu - strip * a.nseg;
    const int h = (int)a.h, w = (int)a.w, x0 = (int)sx * SEG, segw = w - x0 < SEG ? w - x0 : SEG;
    const int y0 = (int)strip * STRIP;
    const size_t row = (size_t)a.w * 3u * SZ;
    const uint8_t* __restrict__ frame = a.src + (size_t)blockIdx.z * a.src_stride;
    uint8_t* __restrict__ out_frame = a.dst + (size_t)blockIdx.z * a.dst_stride;
    short (*pl)[PLANE] = lds[wave];
    const uint32_t t = a.crawl ? ((a.t0 + blockIdx.z) & 3u) : 0u;
    const int l8 = 8 * (int)lane;
    const bool owns = live && l8 < segw;                                        // the lane owns pixels x0 + 8 lane .. + 7 of every row of the strip
    int pu[8], pv[8];                                                           // the delay line: Ur and Vr of the row before
#pragma unroll
    for (int o = 0; o < 8; ++o) pu[o] = pv[o] = 0;

    // Every wave of every workgroup makes STRIP (SIMPLE) or STRIP + 1 (DELAY) trips and meets two barriers in each: a strip that the frame
    // cuts short repeats the last row and stores nothing for it.  Trip 0 is the delay line's first fill: the row above the strip, or for
    // the strip at the top row 1 (row 0 where h == 1)
    for (int it = Dec::line ? 0 : 1; it <= STRIP; ++it) {
        int y = it == 0 ? (y0 == 0 ? (h > 1 ? 1 : 0) : y0 - 1) : y0 + it - 1;
        const bool store = it != 0 && y < h;
        y = y < h ? y : h - 1;
        const Carrier car((uint32_t)y + t);
        const uint8_t* __restrict__ s = frame + (size_t)y * row;

        // step 1: plane index p is pixel x0 - H + p; the lane stages p = 8 lane .. 8 lane + 7 as two groups of four pixels.  A group lies
        // inside the row or outside it (w % 8 == 0, x0 % 8 == 0, H % 4 == 0); one outside is the edge pixel of the group at the edge
        if (l8 < segw + 2 * H) {
            short8 yv, uv, vv;
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
                    int yy, u0, v0;
                    to_yuv(c[0], c[1], c[2], yy, u0, v0);
                    yv[4 * g + i] = (short)yy; uv[4 * g + i] = (short)u0; vv[4 * g + i] = (short)v0;
                }
            }
            *reinterpret_cast<short8*>(&pl[0][l8]) = yv;
            *reinterpret_cast<short8*>(&pl[1][l8]) = uv;
            *reinterpret_cast<short8*>(&pl[2][l8]) = vv;
        }
        __syncthreads();

        // steps 2 - 4: s index j is pixel x0 - R - NOTCH + j = plane index j + ENC; the lane forms j = 8 lane .. 8 lane + 7 from plane
        // entries 8 lane .. 8 lane + 13.  x0 % 4 == 0, so whether entry i carries U or V is a constant of i that the row's rotation swaps:
        // the two planes are read in the order the row asks for, and only the one of U1 / V1 that the phase keeps is formed.  Under
        // svideo the lane also takes the Y0 of its own eight pixels here, so that nothing reads planes 0 - 2 behind the second barrier
        short yq[8];
        {
            constexpr int OFF = 64 - R - NOTCH;                                 // = -(R + NOTCH) mod 4
            const bool swap = (car.rot & 1) != 0;
            const short* odd_plane = swap ? pl[2] : pl[1];                      // entries whose i + OFF is odd: U unless the row swaps
            const short* even_plane = swap ? pl[1] : pl[2];
            short8 to[2], te[2], ty[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                to[k] = *reinterpret_cast<const short8*>(&odd_plane[l8 + 8 * k]);
                te[k] = *reinterpret_cast<const short8*>(&even_plane[l8 + 8 * k]);
                if constexpr (S::crosstalk) ty[k] = *reinterpret_cast<const short8*>(&pl[0][l8 + 8 * k]);
            }
            short8 sv;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                int acc = 8;
#pragma unroll
                for (int k = 0; k <= 2 * ENC; ++k)
                    acc += tri(k, ENC) * (int)(((i + OFF) & 1) ? to[(i + k) >> 3][(i + k) & 7] : te[(i + k) >> 3][(i + k) & 7]);
                const int c = car.factor(i + OFF) * (acc >> 4);
                sv[i] = (short)((S::crosstalk ? (int)ty[(i + ENC) >> 3][(i + ENC) & 7] : 0) + c);
            }
            if constexpr (!S::crosstalk) {
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    const short4 q = *reinterpret_cast<const short4*>(&pl[0][l8 + H + 4 * g]);
#pragma unroll
                    for (int i = 0; i < 4; ++i) yq[4 * g + i] = q[i];
                }
            }
            *reinterpret_cast<short8*>(&pl[3][l8]) = sv;
        }
        __syncthreads();

        // steps 4 - 9: e index i is pixel x0 + 8 lane + i - R = s index 8 lane + i + NOTCH.  The next trip's first barrier stands between
        // these reads of plane 3 and the next write to it
        if (owns) {
            constexpr int NE = 8 + 2 * R, NS = NE + 2 * NOTCH, NV = (NS + 7) / 8, OFF = 64 - R;
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
                d[i] = car.factor(i + OFF) * 2 * e[i];                          // Ud0 where the phase is odd, Vd0 where it is even
            }
            const bool swap = (car.rot & 1) != 0;
            const int vs = car.v * a.st;
            uint32_t od[24 / P::SPD];
            int res[24];
#pragma unroll
            for (int o = 0; o < 8; ++o) {
                int ao = 1 << (C::shift - 1), ae = ao;                          // the taps at odd and at even i + OFF
#pragma unroll
                for (int m = 0; m <= 2 * R; ++m) {
                    if (((o + m + OFF) & 1) != 0) ao += tri(m, R) * d[o + m]; else ae += tri(m, R) * d[o + m];
                }
                const int ud = (swap ? ae : ao) >> C::shift, vd = (swap ? ao : ae) >> C::shift;
                int ur, vr;
                rotate(ud, vd, a.ct, vs, ur, vr);
                int uo = ur, vo = vr;
                if constexpr (Dec::line) {
                    uo = (ur + pu[o] + 1) >> 1; vo = (vr + pv[o] + 1) >> 1;
                    pu[o] = ur; pv[o] = vr;
                }
                int yd;
                if constexpr (S::crosstalk) yd = (int)sq[(o + R + 2) >> 3][(o + R + 2) & 7] - e[o + R]; else yd = (int)yq[o];
                int c[3];
                to_rgb<M>(yd, uo, vo, c);
#pragma unroll
                for (int k = 0; k < 3; ++k) res[3 * o + k] = c[k];
            }
            if (store) {
                constexpr int SPD = P::SPD, OD = 24 / SPD;
#pragma unroll
                for (int j = 0; j < OD; ++j) {
                    uint32_t v = 0u;
#pragma unroll
                    for (int k = 0; k < SPD; ++k) v |= P::bits(res[j * SPD + k]) << (8 * SZ * k);
                    od[j] = v;
                }
                store_dwords<OD>(out_frame + (size_t)y * row + (size_t)(x0 + l8) * 3u * SZ, od);
            }
        }
    }
}

// ---- general: one lane per pixel; the cascade of that pixel in its row and, under DELAY, in the partner row, from clamped loads ----

// steps 1 - 7 of pixel x of row y: Yd, Ur, Vr
template <class S, class C, class P>
__device__ __forceinline__ void pixel_of_row(const Args& a, const typename P::T* __restrict__ frame, int x, int y, uint32_t t, int& yd, int& ur, int& vr) {
    typedef typename P::T T;
    constexpr int R = C::reach, H = R + NOTCH + ENC, NW = 2 * H + 1, NS = 2 * (R + NOTCH) + 1, NE = 2 * R + 1;
    const int w = (int)a.w;
    const T* __restrict__ s = frame + (size_t)y * ((size_t)a.w * 3u);
    const Carrier car((uint32_t)y + t);
    int y0[NW], u0[NW], v0[NW];                                                 // entry p: pixel x - H + p
#pragma unroll
    for (int p = 0; p < NW; ++p) {
        const int xx = x - H + p, xc = xx < 0 ? 0 : (xx >= w ? w - 1 : xx);
        const T* px = s + (size_t)xc * 3u;
        to_yuv(P::code(px[0]), P::code(px[1]), P::code(px[2]), y0[p], u0[p], v0[p]);
    }
    int sg[NS];                                                                 // entry j: pixel x - R - NOTCH + j
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        int au = 8, av = 8;
#pragma unroll
        for (int k = 0; k <= 2 * ENC; ++k) { au += tri(k, ENC) * u0[j + k]; av += tri(k, ENC) * v0[j + k]; }
        const int xx = x - R - NOTCH + j;
        const int c = car.factor(xx) * (car.odd(xx) ? au >> 4 : av >> 4);
        sg[j] = (S::crosstalk ? y0[j + ENC] : 0) + c;
    }
    int au = 1 << (C::shift - 1), av = au;
#pragma unroll
    for (int i = 0; i < NE; ++i) {                                              // entry i: pixel x - R + i
        const int c = sg[i + NOTCH];
        const int e = S::crosstalk ? c - ((sg[i] + 2 * c + sg[i + 2 * NOTCH] + 2) >> 2) : c;
        const int xx = x - R + i;
        const int d = tri(i, R) * car.factor(xx) * 2 * e;
        if (car.odd(xx)) au += d; else av += d;
    }
    yd = S::crosstalk ? (sg[R] + 2 * sg[R + NOTCH] + sg[R + 2 * NOTCH] + 2) >> 2 : y0[H];
    rotate(au >> C::shift, av >> C::shift, a.ct, car.v * a.st, ur, vr);
}

template <class S, class C, class Dec, class P>
__device__ __forceinline__ void pal_general(const Args& a) {
    typedef typename P::T T;
    constexpr int M = sizeof(T) == 1 ? 255 : 1020;
    const int x = (int)(blockIdx.x * BLOCK + threadIdx.x), w = (int)a.w, h = (int)a.h;
    const int y = (int)blockIdx.y;
    if (x >= w) return;
    const T* __restrict__ frame = reinterpret_cast<const T*>(a.src + (size_t)blockIdx.z * a.src_stride);
    const uint32_t t = a.crawl ? ((a.t0 + blockIdx.z) & 3u) : 0u;
    int yd, u, v;
    pixel_of_row<S, C, P>(a, frame, x, y, t, yd, u, v);
    if constexpr (Dec::line) {
        const int yp = y >= 1 ? y - 1 : (h > 1 ? 1 : 0);
        int ydp, up, vp;
        pixel_of_row<S, C, P>(a, frame, x, yp, t, ydp, up, vp);
        u = (u + up + 1) >> 1; v = (v + vp + 1) >> 1;
    }
    int c[3];
    to_rgb<M>(yd, u, v, c);
    T* __restrict__ d = reinterpret_cast<T*>(a.dst + (size_t)blockIdx.z * a.dst_stride) + (size_t)y * ((size_t)a.w * 3u) + (size_t)x * 3u;
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = (T)P::bits(c[k]);
}

template <class S, class C, class Dec, class P, class Path>
__global__ __launch_bounds__(BLOCK) void k_pal(Args a) {
    if constexpr (std::is_same<Path, vec>::value) pal_vec<S, C, Dec, P>(a); else pal_general<S, C, Dec, P>(a);
}

}  // namespace crtfx_pal_impl

using namespace crtfx_pal_impl;

struct crtfx_pal : crtfx_frames::Plan {        // one frame size and sample type on both sides
    int h = 0, w = 0;
    bool half = false, svid = false, wide = false, crawl = false, simple_dec = false;
    int ct = 4096, st = 0;                      // the phase table's entry of the plan's phase
    int64_t first_index = 0;                    // of the run under way: crtfx_pal_run carries it into launch
};

namespace {

using crtfx_frames::Batch;
using crtfx_stage::create_err;
using crtfx_stage::fail;

template <class S, class C, class Dec, class P>
void launch_path(bool fits, dim3 grid, hipStream_t st, const Args& a) {
    if (fits) hipLaunchKernelGGL((k_pal<S, C, Dec, P, vec>), grid, dim3(BLOCK), 0, st, a);
    else hipLaunchKernelGGL((k_pal<S, C, Dec, P, general>), grid, dim3(BLOCK), 0, st, a);
}

template <class S, class C, class Dec>
void launch_pix(const crtfx_pal* p, bool fits, dim3 grid, hipStream_t st, const Args& a) {
    if (p->half) launch_path<S, C, Dec, f16>(fits, grid, st, a); else launch_path<S, C, Dec, u8>(fits, grid, st, a);
}

template <class S, class C>
void launch_decoder(const crtfx_pal* p, bool fits, dim3 grid, hipStream_t st, const Args& a) {
    if (p->simple_dec) launch_pix<S, C, simple>(p, fits, grid, st, a); else launch_pix<S, C, delay>(p, fits, grid, st, a);
}

template <class S>
void launch_chroma(const crtfx_pal* p, bool fits, dim3 grid, hipStream_t st, const Args& a) {
    if (p->wide) launch_decoder<S, soft>(p, fits, grid, st, a); else launch_decoder<S, sharp>(p, fits, grid, st, a);
}

struct U : crtfx_frames::Unit {
    using H = crtfx_pal;
    static constexpr int force_option = CRTFX_PAL_OPT_FORCE_GENERAL;
    static constexpr const char* name = "pal";
    static constexpr bool one_size = true;

    // the vec kernels' conditions (crtfx_pal.h): those of crtfx_signal.h
    static bool vec_fits(const H* p, const Batch& b) {
        if (p->force_general || (p->w & 7)) return false;
        if ((reinterpret_cast<uintptr_t>(b.src) | reinterpret_cast<uintptr_t>(b.dst)) & 3u) return false;
        return b.n <= 1 || !((b.src_stride | b.dst_stride) & 3u);
    }

    static void note_plan(H* p, bool fits, int frames) {
        snprintf(p->plan, sizeof p->plan, "pal=k_pal<%s,%s,%s,%s,%s>;frames=%d", p->svid ? svideo::name : composite::name,
                 p->wide ? soft::name : sharp::name, p->simple_dec ? simple::name : delay::name, p->half ? f16::name : u8::name,
                 fits ? vec::name : general::name, frames);
    }

    static Args make_args(const H* p, bool, const Batch&) {
        Args a{};
        a.h = (uint32_t)p->h; a.w = (uint32_t)p->w;
        a.nseg = (a.w + SEG - 1) / SEG;
        a.units = (a.h + STRIP - 1) / STRIP * a.nseg;                   // below 2^22
        a.crawl = p->crawl ? 1u : 0u;
        a.ct = p->ct; a.st = p->st;
        return a;
    }

    static void launch(const H* p, bool fits, Args& a, int f, unsigned g, hipStream_t st) {
        a.t0 = (uint32_t)((p->first_index + f) & 3);
        const dim3 grid = fits ? dim3((a.units + WAVES - 1) / WAVES, 1, g) : dim3((a.w + BLOCK - 1) / BLOCK, p->h, g);
        if (p->svid) launch_chroma<svideo>(p, fits, grid, st, a); else launch_chroma<composite>(p, fits, grid, st, a);
    }
};

}  // namespace

extern "C" {

const char* crtfx_pal_last_error(const crtfx_pal* p) { return p ? p->err.c_str() : create_err<crtfx_pal>().c_str(); }

int crtfx_pal_phase_table(int degrees, int* c, int* s) {
    if (!c || !s || degrees < -180 || degrees > 180) return CRTFX_E_INVALID;
    const double th = (double)degrees * 3.14159265358979323846 / 180.0;
    *c = (int)llrint(4096.0 * cos(th));
    *s = (int)llrint(4096.0 * sin(th));
    return CRTFX_OK;
}

int crtfx_pal_create(int device, int h, int w, int pix_fmt, int signal, int chroma, int crawl, int decoder, int phase, crtfx_pal** out_plan) {
    using H = crtfx_pal;
    if (const int rc = crtfx_frames::begin_create(out_plan)) return rc;
    if (const int rc = crtfx_frames::check_size<H>("h", h)) return rc;
    if (const int rc = crtfx_frames::check_size<H>("w", w)) return rc;
    if (pix_fmt != CRTFX_PIX_U8 && pix_fmt != CRTFX_PIX_F16) return fail<H>(nullptr, CRTFX_E_INVALID, "unknown pix_fmt %d", pix_fmt);
    if (signal != CRTFX_PAL_COMPOSITE && signal != CRTFX_PAL_SVIDEO) return fail<H>(nullptr, CRTFX_E_INVALID, "unknown signal %d", signal);
    if (chroma != CRTFX_PAL_SHARP && chroma != CRTFX_PAL_SOFT) return fail<H>(nullptr, CRTFX_E_INVALID, "unknown chroma %d", chroma);
    if (crawl != 0 && crawl != 1) return fail<H>(nullptr, CRTFX_E_INVALID, "crawl = %d is neither 0 nor 1", crawl);
    if (decoder != CRTFX_PAL_DELAY && decoder != CRTFX_PAL_SIMPLE) return fail<H>(nullptr, CRTFX_E_INVALID, "unknown decoder %d", decoder);
    if (phase < -180 || phase > 180) return fail<H>(nullptr, CRTFX_E_INVALID, "phase = %d outside -180..180", phase);
    return crtfx_frames::new_plan<U>(device, out_plan, [&](H* p) {
        p->h = h; p->w = w;
        p->half = pix_fmt == CRTFX_PIX_F16; p->svid = signal == CRTFX_PAL_SVIDEO; p->wide = chroma == CRTFX_PAL_SOFT; p->crawl = crawl != 0;
        p->simple_dec = decoder == CRTFX_PAL_SIMPLE;
        (void)crtfx_pal_phase_table(phase, &p->ct, &p->st);
        p->src_bps = p->dst_bps = p->half ? 2 : 1;
        p->src_bytes = p->dst_bytes = (size_t)h * w * 3 * p->src_bps;
        return CRTFX_OK;
    });
}

int crtfx_pal_destroy(crtfx_pal* p) { return crtfx_frames::destroy(p); }

int crtfx_pal_set_option(crtfx_pal* p, int option, int value) { return crtfx_frames::set_option<U>(p, option, value); }

int crtfx_pal_last_plan(crtfx_pal* p, char* buf, size_t n) { return crtfx_frames::last_plan(p, buf, n); }

int crtfx_pal_run(crtfx_pal* p, int64_t first_index, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n,
                  void* stream) {
    if (!p) return CRTFX_E_INVALID;
    if (first_index < 0) return fail(p, CRTFX_E_INVALID, "first_index = %lld is negative", (long long)first_index);
    p->first_index = first_index;
    return crtfx_frames::run<U>(p, Batch{nullptr, src_base, src_stride_bytes, dst_base, dst_stride_bytes, n}, stream);
}

}  // extern "C"
