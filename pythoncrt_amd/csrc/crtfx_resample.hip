// crtfx_resample.hip — the filtered resampler of libcrtfx.so (include/crtfx_resample.h): Pillow's 8-bit two-pass resize with signed taps (BOX,
// BILINEAR, HAMMING, BICUBIC, LANCZOS), h x w x 3 RGB frames of uint8 or of halves on the quarter-code scale, on the device.  A translation
// unit of its own: it shares no kernel, table or handle with the effect chain or with the two BILINEAR stages whose structure it follows.
// Here are its kernels, its handle, its two-option set_option and what the resize stages' host skeleton (crtfx_resize_host.h, host templates
// only) asks of a unit; create, run and the other entry points are that skeleton's.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "crtfx_resample.h"
#include "crtfx_resize_host.h"

namespace crtfx_resample_impl {

constexpr int BLOCK = 256;
constexpr int PREC = 22;                       // Pillow's PRECISION_BITS (32 - 8 - 2)
constexpr int HALF = 1 << (PREC - 1);

struct Axis { const int32_t* min; const int32_t* count; const int32_t* k; int ksize; };

struct Args {
    const unsigned char* src; size_t src_stride;   // strides in bytes
    unsigned char* dst; size_t dst_stride;
    int sh, sw, dh, dw;
    Axis x, y;
    int TH, TW;                // output rows / columns per tile
    int P, HP;                 // LDS bytes per staged source row / per row of the horizontal result (multiples of 4)
    int nr_max;                // source rows of the tallest tile
    int sh_stage, sh_h, sh_v;  // log2 of the work items per row of the three phases (power-of-two rows: item -> (row, column) is a shift and a mask)
};

// q = rint_to_even(min(max(4 f, 0), 1020)), NaN -> 0: the quantiser of crtfx_resize16.hip, word for word
__device__ __forceinline__ unsigned quantise(unsigned bits16) {
    float t = 4.0f * (float)__builtin_bit_cast(_Float16, (unsigned short)bits16);
    t = t > 0.0f ? t : 0.0f;
    t = t < 1020.0f ? t : 1020.0f;
    return (unsigned)(int)rintf(t);
}

// the half bit pattern of quarter code q, q / 4 on the 0..255 scale: exact, every quarter code is a half (no rounding occurs)
__device__ __forceinline__ unsigned half_bits(unsigned q) { return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)((float)q * 0.25f)); }

// The sum of one output sample.  Three forms with one interface: tap(k, v) adds k * v, out() is clamp((2^21 + sum) >> 22, 0, top).
struct AccU8 {                                  // samples 0..255: every partial sum fits int32 (the row rule of crtfx_resample_create)
    int a = HALF;
    __device__ __forceinline__ void tap(int k, unsigned v) { a += __mul24(k, (int)v); }
    __device__ __forceinline__ unsigned out() const { return (unsigned)max(0, min(a >> PREC, 255)); }
};
struct AccAB {                                  // quarter codes 0..1020: A over q >> 2 (0..255), B over q & 3; 4 A + B is the int64 sum
    int A = 0, B = 0;
    __device__ __forceinline__ void tap(int k, unsigned v) { A += __mul24(k, (int)(v >> 2)); B += __mul24(k, (int)(v & 3u)); }
    __device__ __forceinline__ unsigned out() const {
        const long long s = ((long long)A << 2) + (long long)B + HALF;
        const long long q = s >> PREC;
        return (unsigned)(q < 0 ? 0 : (q > 1020 ? 1020 : q));
    }
};
struct Acc64 {                                  // the same sum, one 64-bit multiply-add per tap (CRTFX_RESAMPLE_OPT_ACC64)
    long long a = HALF;
    __device__ __forceinline__ void tap(int k, unsigned v) { a += (long long)k * (long long)(int)v; }
    __device__ __forceinline__ unsigned out() const {
        const long long q = a >> PREC;
        return (unsigned)(q < 0 ? 0 : (q > 1020 ? 1020 : q));
    }
};

// E: the sample type in memory (uint8_t bytes; uint16_t half bit patterns, quarter codes once staged).  ACC: the sum above.
template <typename E> struct Px;
template <> struct Px<uint8_t> {
    static __device__ __forceinline__ unsigned load(unsigned v) { return v; }                 // a sample read from memory -> what a tap multiplies
    static __device__ __forceinline__ unsigned stage(unsigned dword) { return dword; }        // a dword of samples from memory -> LDS
    static __device__ __forceinline__ unsigned store(unsigned q) { return q; }                // a result -> the sample written to memory
};
template <> struct Px<uint16_t> {
    static __device__ __forceinline__ unsigned load(unsigned v) { return quantise(v); }
    static __device__ __forceinline__ unsigned stage(unsigned dword) { return quantise(dword & 0xFFFFu) | (quantise(dword >> 16) << 16); }
    static __device__ __forceinline__ unsigned store(unsigned q) { return half_bits(q); }
};

// One block = TH output rows x TW output columns of one frame.
//   phase 0  the tile's slice of the six tables -> LDS
//   phase 1  the source rows / columns its taps reach -> LDS, one thread per aligned dword (a row keeps its global address modulo 4, so a
//            dword in LDS is a dword in memory; only a dword that sticks out of the frame's own bytes is assembled from byte loads); halves
//            become quarter codes here
//   phase 2  horizontal pass, one thread per (source row, output pixel): three sums per tap, result -> LDS as samples
//   phase 3  vertical pass, one thread per ALIGNED dword of an output row (the samples in front of the first and behind the last aligned
//            dword of the tile's row segment are single items): per tap two LDS dwords funnel-shifted to the row's phase
template <typename E, typename ACC>
__global__ __launch_bounds__(BLOCK) void k_resample_fused(Args a) {
    constexpr int BPS = (int)sizeof(E);         // bytes per sample
    constexpr int EPD = 4 / BPS;                // samples per dword
    constexpr unsigned EMASK = BPS == 1 ? 0xFFu : 0xFFFFu;
    extern __shared__ __align__(16) unsigned char lds[];
    const int tid = threadIdx.x;
    const int ox0 = blockIdx.x * a.TW, oy0 = blockIdx.y * a.TH;
    const int ow = min(a.TW, a.dw - ox0), oh = min(a.TH, a.dh - oy0);
    const unsigned char* fsrc = a.src + (size_t)blockIdx.z * a.src_stride;
    const unsigned char* fend = fsrc + (size_t)a.sh * a.sw * 3 * BPS;
    unsigned char* fdst = a.dst + (size_t)blockIdx.z * a.dst_stride;

    int* s_xmin = reinterpret_cast<int*>(lds);
    int* s_xcnt = s_xmin + a.TW;
    int* s_kx = s_xcnt + a.TW;
    int* s_ymin = s_kx + a.TW * a.x.ksize;
    int* s_ycnt = s_ymin + a.TH;
    int* s_ky = s_ycnt + a.TH;
    unsigned* S = reinterpret_cast<unsigned*>(s_ky + a.TH * a.y.ksize);
    unsigned* Hb = S + (size_t)a.nr_max * (a.P >> 2);

    // min and min + count are non-decreasing (checked by crtfx_resample_create): the tile's source window is first tap .. last tap
    const int sx0 = a.x.min[ox0], sx1 = a.x.min[ox0 + ow - 1] + a.x.count[ox0 + ow - 1];
    const int sy0 = a.y.min[oy0], sy1 = a.y.min[oy0 + oh - 1] + a.y.count[oy0 + oh - 1];
    const int nr = sy1 - sy0, sb = (sx1 - sx0) * 3 * BPS;

    for (int i = tid; i < ow; i += BLOCK) { s_xmin[i] = a.x.min[ox0 + i] - sx0; s_xcnt[i] = a.x.count[ox0 + i]; }
    for (int i = tid; i < ow * a.x.ksize; i += BLOCK) s_kx[i] = a.x.k[(size_t)ox0 * a.x.ksize + i];
    for (int i = tid; i < oh; i += BLOCK) { s_ymin[i] = a.y.min[oy0 + i] - sy0; s_ycnt[i] = a.y.count[oy0 + i]; }
    for (int i = tid; i < oh * a.y.ksize; i += BLOCK) s_ky[i] = a.y.k[(size_t)oy0 * a.y.ksize + i];

    const size_t srow = (size_t)a.sw * 3 * BPS;
    for (int idx = tid; idx < (nr << a.sh_stage); idx += BLOCK) {
        const int r = idx >> a.sh_stage, d = idx & ((1 << a.sh_stage) - 1);
        const unsigned char* g = fsrc + (size_t)(sy0 + r) * srow + (size_t)sx0 * 3 * BPS;
        const unsigned lead = (unsigned)(reinterpret_cast<uintptr_t>(g) & 3u);
        if (d < (int)((lead + sb + 3) >> 2)) {
            const unsigned char* p = g - lead + 4 * d;
            unsigned v;
            if (p >= fsrc && p + 4 <= fend) {
                v = *reinterpret_cast<const unsigned*>(p);
            } else {
                v = 0;
                for (int e = 0; e < 4; ++e)
                    if (p + e >= fsrc && p + e < fend) v |= (unsigned)p[e] << (8 * e);
            }
            S[r * (a.P >> 2) + d] = Px<E>::stage(v);
        }
    }
    __syncthreads();

    const unsigned char* Sb = reinterpret_cast<const unsigned char*>(S);
    unsigned char* Hbb = reinterpret_cast<unsigned char*>(Hb);
    for (int idx = tid; idx < (nr << a.sh_h); idx += BLOCK) {
        const int r = idx >> a.sh_h, p = idx & ((1 << a.sh_h) - 1);
        if (p < ow) {
            const unsigned lead = (unsigned)(reinterpret_cast<uintptr_t>(fsrc + (size_t)(sy0 + r) * srow + (size_t)sx0 * 3 * BPS) & 3u);
            const E* s = reinterpret_cast<const E*>(Sb + r * a.P + lead) + s_xmin[p] * 3;      // half frames: lead is 0 or 2
            const int* k = s_kx + p * a.x.ksize;
            const int cnt = s_xcnt[p];
            ACC a0, a1, a2;
            for (int t = 0; t < cnt; ++t) {
                const int kk = k[t];
                a0.tap(kk, s[3 * t]);
                a1.tap(kk, s[3 * t + 1]);
                a2.tap(kk, s[3 * t + 2]);
            }
            E* o = reinterpret_cast<E*>(Hbb + r * a.HP) + p * 3;
            o[0] = (E)a0.out(); o[1] = (E)a1.out(); o[2] = (E)a2.out();
        }
    }
    __syncthreads();

    const int nb = ow * 3 * BPS;                              // bytes of the tile's row segment
    const size_t drow = (size_t)a.dw * 3 * BPS;
    for (int idx = tid; idx < (oh << a.sh_v); idx += BLOCK) {
        const int y = idx >> a.sh_v, i = idx & ((1 << a.sh_v) - 1);
        unsigned char* g = fdst + (size_t)(oy0 + y) * drow + (size_t)ox0 * 3 * BPS;
        const int lead = min(nb, (int)((4u - (unsigned)(reinterpret_cast<uintptr_t>(g) & 3u)) & 3u));   // bytes in front of the first aligned dword
        const int nd = (nb - lead) >> 2;
        const int* k = s_ky + y * a.y.ksize;
        const int cnt = s_ycnt[y];
        const int r0 = s_ymin[y];
        if (i < nd) {
            const int o = lead + 4 * i;                       // byte offset in the tile's row; o + 3 < nb
            const unsigned* h = Hb + r0 * (a.HP >> 2) + (o >> 2);
            const unsigned sh8 = (unsigned)(o & 3) * 8u;
            ACC acc[EPD];
            for (int t = 0; t < cnt; ++t) {
                const int kk = k[t];
                unsigned v = h[0];
                if (sh8) v = (v >> sh8) | (h[1] << (32u - sh8));   // h[1] lies inside the row's pitch (HP = round4(3 b * TW) + 4)
#pragma unroll
                for (int e = 0; e < EPD; ++e) acc[e].tap(kk, (v >> (8 * BPS * e)) & EMASK);
                h += a.HP >> 2;
            }
            // The dword is built from its last sample down, (w << 8 b) + sample.  Written as w |= sample << (8 b e), two of the uint8 clamps
            // are paired into one v_ashr_pk_u8_i32, whose 16-bit result the compiler then ORs as a whole register: on the MI355X byte 2 of
            // every dword came out with the upper bits of the coefficient that register held before (0x40 under the box filter).  This
            // form keeps each clamp a v_med3_i32; tests/test_resample_tables.py holds the build to that.
            unsigned w = Px<E>::store(acc[EPD - 1].out());
#pragma unroll
            for (int e = EPD - 2; e >= 0; --e) w = (w << (8 * BPS)) + Px<E>::store(acc[e].out());
            *reinterpret_cast<unsigned*>(g + o) = w;
        } else if (i < nd + (nb - 4 * nd) / BPS) {            // the samples outside the aligned dwords
            const int e = (i - nd) * BPS;
            const int o = e < lead ? e : 4 * nd + e;          // the head, then the tail behind the last aligned dword
            const E* h = reinterpret_cast<const E*>(Hbb + r0 * a.HP + o);
            ACC acc;
            for (int t = 0; t < cnt; ++t) { acc.tap(k[t], h[0]); h += a.HP / BPS; }
            *reinterpret_cast<E*>(g + o) = (E)Px<E>::store(acc.out());
        }
    }
}

// General path, any tap count.  Horizontal pass: one thread per output pixel of a source row, taps read from memory (halves quantised there).
template <typename E, typename ACC>
__global__ __launch_bounds__(BLOCK) void k_resample_h(const E* src, size_t src_stride, E* tmp, int sh, int sw, int dw, Axis x) {
    const int px = blockIdx.x * BLOCK + threadIdx.x;
    if (px >= dw) return;
    const E* s = src + (size_t)blockIdx.z * src_stride + ((size_t)blockIdx.y * sw + x.min[px]) * 3;
    const int32_t* k = x.k + (size_t)px * x.ksize;
    const int cnt = x.count[px];
    ACC a0, a1, a2;
    for (int t = 0; t < cnt; ++t) {
        const int kk = k[t];
        a0.tap(kk, Px<E>::load(s[3 * t]));
        a1.tap(kk, Px<E>::load(s[3 * t + 1]));
        a2.tap(kk, Px<E>::load(s[3 * t + 2]));
    }
    E* o = tmp + (((size_t)blockIdx.z * sh + blockIdx.y) * dw + px) * 3;
    o[0] = (E)a0.out(); o[1] = (E)a1.out(); o[2] = (E)a2.out();
}

// Vertical pass: one thread per output sample of an output row (consecutive lanes, consecutive samples).
template <typename E, typename ACC>
__global__ __launch_bounds__(BLOCK) void k_resample_v(const E* tmp, E* dst, size_t dst_stride, int sh, int dw, Axis y) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    const size_t row = (size_t)dw * 3;
    if ((size_t)j >= row) return;
    const int oy = blockIdx.y;
    const E* s = tmp + ((size_t)blockIdx.z * sh + y.min[oy]) * row + j;
    const int32_t* k = y.k + (size_t)oy * y.ksize;
    const int cnt = y.count[oy];
    ACC acc;
    for (int t = 0; t < cnt; ++t) { acc.tap(k[t], s[0]); s += row; }
    dst[(size_t)blockIdx.z * dst_stride + (size_t)oy * row + j] = (E)Px<E>::store(acc.out());
}

}  // namespace crtfx_resample_impl

using namespace crtfx_resample_impl;

struct crtfx_resample : crtfx_resize::Plan<Axis, Args> {
    bool acc64 = false;
};

namespace {

using crtfx_resize::fail;

template <typename E, typename ACC>
void launch_as(crtfx_resample* p, bool fused, const unsigned char* src, size_t ss, unsigned char* dst, size_t ds, int g, hipStream_t st) {
    if (fused) {
        Args a = p->fused;
        a.x = p->x; a.y = p->y;
        a.src = src; a.src_stride = ss;
        a.dst = dst; a.dst_stride = ds;
        dim3 grid((p->dw + a.TW - 1) / a.TW, (p->dh + a.TH - 1) / a.TH, g);
        hipLaunchKernelGGL((k_resample_fused<E, ACC>), grid, dim3(BLOCK), (size_t)p->lds_bytes, st, a);
    } else {
        hipLaunchKernelGGL((k_resample_h<E, ACC>), dim3((p->dw + BLOCK - 1) / BLOCK, p->sh, g), dim3(BLOCK), 0, st,
                           reinterpret_cast<const E*>(src), ss / sizeof(E), static_cast<E*>(p->scratch), p->sh, p->sw, p->dw, p->x);
        hipLaunchKernelGGL((k_resample_v<E, ACC>), dim3((p->dw * 3 + BLOCK - 1) / BLOCK, p->dh, g), dim3(BLOCK), 0, st,
                           static_cast<const E*>(p->scratch), reinterpret_cast<E*>(dst), ds / sizeof(E), p->sh, p->dw, p->y);
    }
}

// what crtfx_resize_host.h asks of a unit
struct Unit {
    using H = crtfx_resample;
    static const char* name() { return "resample"; }
    static int bps(int pix_fmt) { return pix_fmt == CRTFX_PIX_U8 ? 1 : 2; }

    static int check_pix_fmt(int pix_fmt) {
        if (pix_fmt != CRTFX_PIX_U8 && pix_fmt != CRTFX_PIX_F16) return fail<H>(nullptr, CRTFX_E_INVALID, "unknown pixel format %d", pix_fmt);
        return CRTFX_OK;
    }

    // the rule crtfx_resample.h states for a row; the accumulators' ranges rest on it
    static const char* check_row(const int32_t* k, int cnt) {
        long long pos = 0, neg = 0;
        for (int t = 0; t < cnt; ++t) {
            if (k[t] < -(1 << 23) || k[t] >= (1 << 23)) return "a coefficient is outside [-2^23, 2^23)";
            if (k[t] > 0) pos += k[t]; else neg += k[t];
        }
        if ((long long)HALF + 255 * pos >= (1LL << 31) || 255 * neg <= -(1LL << 31))
            return "a row's accumulator could leave int32 (2^21 + 255 * sum(k > 0) < 2^31 and 255 * sum(k < 0) > -2^31)";
        return nullptr;
    }

    static void lds_rows(const H* p, long long nc, int cols, long long* P, long long* HP, int* v_items) {
        const long long b = p->bps;
        *P = (3 * b * nc + 3 + 3) & ~3LL;
        *HP = ((3 * b * cols + 3) & ~3LL) + 4;
        *v_items = (3 * (int)b * cols) / 4 + 6;                   // aligned dwords of a row segment + at most three samples on either side
    }

    static void note_plan(H* p, int frames) {
        const char* px = p->bps == 1 ? "u8" : "half";
        const char* acc = p->acc64 ? ";acc=i64" : "";
        if (p->fused_fits && !p->force_general)
            snprintf(p->plan, sizeof p->plan, "resample=k_resample_fused<%s,rows=%d,cols=%d>;lds=%d;frames=%d%s", px, p->fused.TH, p->fused.TW, p->lds_bytes, frames, acc);
        else
            snprintf(p->plan, sizeof p->plan, "resample=k_resample_h+k_resample_v<%s>;frames=%d%s", px, frames, acc);
    }

    static int check_alignment(H* p, const void* src, size_t src_stride_bytes, const void* dst, size_t dst_stride_bytes) {
        if (p->bps == 2 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | src_stride_bytes | dst_stride_bytes) & 1u))
            return fail(p, CRTFX_E_INVALID, "frame bases and strides of half frames must be even (16-bit elements)");
        return CRTFX_OK;
    }

    static void launch(H* p, bool fused, const unsigned char* src, size_t ss, unsigned char* dst, size_t ds, int g, hipStream_t st) {
        if (p->bps == 1) launch_as<uint8_t, AccU8>(p, fused, src, ss, dst, ds, g, st);
        else if (p->acc64) launch_as<uint16_t, Acc64>(p, fused, src, ss, dst, ds, g, st);
        else launch_as<uint16_t, AccAB>(p, fused, src, ss, dst, ds, g, st);
    }
};

}  // namespace

extern "C" {

const char* crtfx_resample_last_error(const crtfx_resample* p) { return p ? p->err.c_str() : crtfx_resize::create_err<crtfx_resample>().c_str(); }

int crtfx_resample_create(int device, int src_h, int src_w, int dst_h, int dst_w, int pix_fmt,
                          const int32_t* x_min, const int32_t* x_count, const int32_t* x_k, int x_ksize,
                          const int32_t* y_min, const int32_t* y_count, const int32_t* y_k, int y_ksize, crtfx_resample** out_plan) {
    return crtfx_resize::create<Unit>(device, src_h, src_w, dst_h, dst_w, pix_fmt, x_min, x_count, x_k, x_ksize, y_min, y_count, y_k, y_ksize, out_plan);
}

int crtfx_resample_destroy(crtfx_resample* p) { return crtfx_resize::destroy(p); }

// two options: the entry point is the unit's own
int crtfx_resample_set_option(crtfx_resample* p, int option, int value) {
    if (!p) return CRTFX_E_INVALID;
    if (option != CRTFX_RESAMPLE_OPT_FORCE_GENERAL && option != CRTFX_RESAMPLE_OPT_ACC64) return fail(p, CRTFX_E_INVALID, "unknown resample option %d", option);
    if (value != 0 && value != 1) return fail(p, CRTFX_E_INVALID, "option %d takes 0 or 1, got %d", option, value);
    if (option == CRTFX_RESAMPLE_OPT_ACC64) {
        if (p->bps != 2) return fail(p, CRTFX_E_INVALID, "ACC64 applies to half frames only (a uint8 sum fits int32)");
        p->acc64 = value != 0;
    } else {
        p->force_general = value != 0;
    }
    Unit::note_plan(p, 0);
    return CRTFX_OK;
}

int crtfx_resample_last_plan(crtfx_resample* p, char* buf, size_t n) { return crtfx_resize::last_plan(p, buf, n); }

int crtfx_resample_run(crtfx_resample* p, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream) {
    return crtfx_resize::run<Unit>(p, src_base, src_stride_bytes, dst_base, dst_stride_bytes, n, stream);
}

}  // extern "C"
