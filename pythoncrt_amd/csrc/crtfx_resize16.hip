// crtfx_resize16.hip — the half resampler of libcrtfx.so (include/crtfx_resize16.h): Pillow's 8-bit BILINEAR resize on the quarter-code scale,
// h x w x 3 half RGB frames on the device.  A translation unit of its own: it shares no kernel, table or handle with the effect chain or with
// the ingest stage whose structure it follows.  Here are its kernels, its handle and what the resize stages' host skeleton
// (crtfx_resize_host.h, host templates only) asks of a unit; create, run and the other entry points are that skeleton's.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "crtfx_resize16.h"
#include "crtfx_resize_host.h"

namespace crtfx_resize16_impl {

constexpr int BLOCK = 256;
constexpr int PREC = 22;                       // Pillow's PRECISION_BITS (32 - 8 - 2)
constexpr unsigned HALF = 1u << (PREC - 1);
constexpr unsigned QMAX = 1020;                // the largest quarter code (255.0 on the half scale)

struct Axis { const int32_t* min; const int32_t* count; const int32_t* k; int ksize; };

struct Args {
    const uint16_t* src; size_t src_stride;    // strides in 16-bit elements
    uint16_t* dst; size_t dst_stride;
    int sh, sw, dh, dw;
    Axis x, y;
    int TH, TW;                // output rows / columns per tile
    int P, HP;                 // LDS bytes per staged source row / per row of the horizontal result (multiples of 4)
    int nr_max;                // source rows of the tallest tile
    int sh_stage, sh_h, sh_v;  // log2 of the work items per row of the three phases (power-of-two rows: item -> (row, column) is a shift and a mask)
};

// q = rint_to_even(min(max(4 f, 0), 1020)), NaN -> 0: crtfx_egress10's quantiser (crtfx_deep.hip), word for word
__device__ __forceinline__ unsigned quantise(unsigned bits16) {
    float t = 4.0f * (float)__builtin_bit_cast(_Float16, (unsigned short)bits16);
    t = t > 0.0f ? t : 0.0f;
    t = t < 1020.0f ? t : 1020.0f;
    return (unsigned)(int)rintf(t);
}

// the half bit pattern of quarter code q, q / 4 on the 0..255 scale: exact, every quarter code is a half (no rounding occurs)
__device__ __forceinline__ unsigned half_bits(unsigned q) { return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)((float)q * 0.25f)); }

__device__ __forceinline__ unsigned clampq(unsigned acc) { return min(acc >> PREC, QMAX); }

// 0 or 1: the 16-bit elements between the dword boundary at or below p and p (every frame base is even)
__device__ __forceinline__ unsigned lead_of(const uint16_t* p) { return (unsigned)(reinterpret_cast<uintptr_t>(p) >> 1) & 1u; }

// One block = TH output rows x TW output columns of one frame.
//   phase 0  the tile's slice of the six tables -> LDS
//   phase 1  the source rows / columns its taps reach -> LDS as quarter codes, one thread per aligned dword of two halves (a row keeps its
//            global address modulo 4, so a dword in LDS is a dword in memory; only a dword that sticks out of the frame's own bytes is
//            assembled from 16-bit loads)
//   phase 2  horizontal pass, one thread per (source row, output pixel): three 24-bit multiply-adds per tap, uint16 result -> LDS
//   phase 3  vertical pass, one thread per ALIGNED dword of an output row (the half in front of the first and behind the last aligned
//            dword of the tile's row segment is a single item): two 24-bit multiply-adds per tap, one dword store of two halves
__global__ __launch_bounds__(BLOCK) void k_resize16_fused(Args a) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int tid = threadIdx.x;
    const int ox0 = blockIdx.x * a.TW, oy0 = blockIdx.y * a.TH;
    const int ow = min(a.TW, a.dw - ox0), oh = min(a.TH, a.dh - oy0);
    const uint16_t* fsrc = a.src + (size_t)blockIdx.z * a.src_stride;
    const uint16_t* fend = fsrc + (size_t)a.sh * a.sw * 3;
    uint16_t* fdst = a.dst + (size_t)blockIdx.z * a.dst_stride;

    int* s_xmin = reinterpret_cast<int*>(lds);
    int* s_xcnt = s_xmin + a.TW;
    int* s_kx = s_xcnt + a.TW;
    int* s_ymin = s_kx + a.TW * a.x.ksize;
    int* s_ycnt = s_ymin + a.TH;
    int* s_ky = s_ycnt + a.TH;
    unsigned* S = reinterpret_cast<unsigned*>(s_ky + a.TH * a.y.ksize);
    unsigned* Hb = S + (size_t)a.nr_max * (a.P >> 2);

    // min and min + count are non-decreasing (checked by crtfx_resize16_create): the tile's source window is first tap .. last tap
    const int sx0 = a.x.min[ox0], sx1 = a.x.min[ox0 + ow - 1] + a.x.count[ox0 + ow - 1];
    const int sy0 = a.y.min[oy0], sy1 = a.y.min[oy0 + oh - 1] + a.y.count[oy0 + oh - 1];
    const int nr = sy1 - sy0, ne = (sx1 - sx0) * 3;

    for (int i = tid; i < ow; i += BLOCK) { s_xmin[i] = a.x.min[ox0 + i] - sx0; s_xcnt[i] = a.x.count[ox0 + i]; }
    for (int i = tid; i < ow * a.x.ksize; i += BLOCK) s_kx[i] = a.x.k[(size_t)ox0 * a.x.ksize + i];
    for (int i = tid; i < oh; i += BLOCK) { s_ymin[i] = a.y.min[oy0 + i] - sy0; s_ycnt[i] = a.y.count[oy0 + i]; }
    for (int i = tid; i < oh * a.y.ksize; i += BLOCK) s_ky[i] = a.y.k[(size_t)oy0 * a.y.ksize + i];

    const size_t srow = (size_t)a.sw * 3;
    for (int idx = tid; idx < (nr << a.sh_stage); idx += BLOCK) {
        const int r = idx >> a.sh_stage, d = idx & ((1 << a.sh_stage) - 1);
        const uint16_t* g = fsrc + (size_t)(sy0 + r) * srow + (size_t)sx0 * 3;
        const unsigned lead = lead_of(g);
        if (d < (int)((lead + ne + 1) >> 1)) {
            const uint16_t* p = g - lead + 2 * d;
            unsigned lo = 0, hi = 0;
            if (p >= fsrc && p + 2 <= fend) {
                const unsigned v = *reinterpret_cast<const unsigned*>(p);
                lo = v & 0xFFFFu; hi = v >> 16;
            } else {
                if (p >= fsrc && p < fend) lo = p[0];
                if (p + 1 >= fsrc && p + 1 < fend) hi = p[1];
            }
            S[r * (a.P >> 2) + d] = quantise(lo) | (quantise(hi) << 16);
        }
    }
    __syncthreads();

    const uint16_t* Sq = reinterpret_cast<const uint16_t*>(S);
    uint16_t* Hq = reinterpret_cast<uint16_t*>(Hb);
    for (int idx = tid; idx < (nr << a.sh_h); idx += BLOCK) {
        const int r = idx >> a.sh_h, p = idx & ((1 << a.sh_h) - 1);
        if (p < ow) {
            const unsigned lead = lead_of(fsrc + (size_t)(sy0 + r) * srow + (size_t)sx0 * 3);
            const uint16_t* s = Sq + r * (a.P >> 1) + lead + s_xmin[p] * 3;
            const int* k = s_kx + p * a.x.ksize;
            const int cnt = s_xcnt[p];
            unsigned a0 = HALF, a1 = HALF, a2 = HALF;
            for (int t = 0; t < cnt; ++t) {
                const unsigned kk = (unsigned)k[t];
                a0 += __umul24(kk, s[3 * t]);
                a1 += __umul24(kk, s[3 * t + 1]);
                a2 += __umul24(kk, s[3 * t + 2]);
            }
            uint16_t* o = Hq + r * (a.HP >> 1) + p * 3;
            o[0] = (uint16_t)clampq(a0); o[1] = (uint16_t)clampq(a1); o[2] = (uint16_t)clampq(a2);
        }
    }
    __syncthreads();

    const int nb = ow * 3;
    const size_t drow = (size_t)a.dw * 3;
    for (int idx = tid; idx < (oh << a.sh_v); idx += BLOCK) {
        const int y = idx >> a.sh_v, i = idx & ((1 << a.sh_v) - 1);
        uint16_t* g = fdst + (size_t)(oy0 + y) * drow + (size_t)ox0 * 3;
        const int lead = min(nb, (int)lead_of(g));            // lead_of(g) halves stand in front of the first aligned dword
        const int nd = (nb - lead) >> 1;
        const int* k = s_ky + y * a.y.ksize;
        const int cnt = s_ycnt[y];
        const uint16_t* h0 = Hq + s_ymin[y] * (a.HP >> 1);
        if (i < nd) {
            const int o = lead + 2 * i;                       // element offset in the tile's row; o + 1 < nb
            const uint16_t* h = h0 + o;
            unsigned a0 = HALF, a1 = HALF;
            for (int t = 0; t < cnt; ++t) {
                const unsigned kk = (unsigned)k[t];
                a0 += __umul24(kk, h[0]);
                a1 += __umul24(kk, h[1]);
                h += a.HP >> 1;
            }
            *reinterpret_cast<unsigned*>(g + o) = half_bits(clampq(a0)) | (half_bits(clampq(a1)) << 16);
        } else if (i < nb - nd) {                             // nb - 2 * nd single halves
            const int e = i - nd;
            const int o = e < lead ? e : 2 * nd + e;          // the head, then the tail behind the last aligned dword
            const uint16_t* h = h0 + o;
            unsigned acc = HALF;
            for (int t = 0; t < cnt; ++t) { acc += __umul24((unsigned)k[t], h[0]); h += a.HP >> 1; }
            g[o] = (uint16_t)half_bits(clampq(acc));
        }
    }
}

// General path, any tap count.  Horizontal pass: one thread per output pixel of a source row, taps read from memory and quantised there.
__global__ __launch_bounds__(BLOCK) void k_resize16_h(const uint16_t* src, size_t src_stride, uint16_t* tmp, int sh, int sw, int dw, Axis x) {
    const int px = blockIdx.x * BLOCK + threadIdx.x;
    if (px >= dw) return;
    const uint16_t* s = src + (size_t)blockIdx.z * src_stride + ((size_t)blockIdx.y * sw + x.min[px]) * 3;
    const int32_t* k = x.k + (size_t)px * x.ksize;
    const int cnt = x.count[px];
    unsigned a0 = HALF, a1 = HALF, a2 = HALF;
    for (int t = 0; t < cnt; ++t) {
        const unsigned kk = (unsigned)k[t];
        a0 += __umul24(kk, quantise(s[3 * t]));
        a1 += __umul24(kk, quantise(s[3 * t + 1]));
        a2 += __umul24(kk, quantise(s[3 * t + 2]));
    }
    uint16_t* o = tmp + (((size_t)blockIdx.z * sh + blockIdx.y) * dw + px) * 3;
    o[0] = (uint16_t)clampq(a0); o[1] = (uint16_t)clampq(a1); o[2] = (uint16_t)clampq(a2);
}

// Vertical pass: one thread per output half of an output row (consecutive lanes, consecutive halves).
__global__ __launch_bounds__(BLOCK) void k_resize16_v(const uint16_t* tmp, uint16_t* dst, size_t dst_stride, int sh, int dw, Axis y) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    const size_t row = (size_t)dw * 3;
    if ((size_t)j >= row) return;
    const int oy = blockIdx.y;
    const uint16_t* s = tmp + ((size_t)blockIdx.z * sh + y.min[oy]) * row + j;
    const int32_t* k = y.k + (size_t)oy * y.ksize;
    const int cnt = y.count[oy];
    unsigned acc = HALF;
    for (int t = 0; t < cnt; ++t) { acc += __umul24((unsigned)k[t], s[0]); s += row; }
    dst[(size_t)blockIdx.z * dst_stride + (size_t)oy * row + j] = (uint16_t)half_bits(clampq(acc));
}

}  // namespace crtfx_resize16_impl

using namespace crtfx_resize16_impl;

struct crtfx_resize16 : crtfx_resize::Plan<Axis, Args> {};

namespace {

using crtfx_resize::fail;

// what crtfx_resize_host.h asks of a unit
struct Unit {
    using H = crtfx_resize16;
    static constexpr int force_option = CRTFX_RESIZE16_OPT_FORCE_GENERAL;
    static const char* name() { return "resize16"; }
    static int bps(int) { return 2; }

    static int check_pix_fmt(int pix_fmt) {
        if (pix_fmt == CRTFX_PIX_U8) return fail<H>(nullptr, CRTFX_E_UNSUPPORTED, "only half RGB frames are resized here (uint8 frames have crtfx_ingest_*)");
        if (pix_fmt != CRTFX_PIX_F16) return fail<H>(nullptr, CRTFX_E_INVALID, "unknown pixel format %d", pix_fmt);
        return CRTFX_OK;
    }

    // the coefficient rule of crtfx_ingest.h, and the accumulator bound of crtfx_resize16.h
    static const char* check_row(const int32_t* k, int cnt) {
        unsigned long long sum = 0;
        for (int t = 0; t < cnt; ++t) {
            if (k[t] < 0 || k[t] >= (1 << 24)) return "a coefficient is outside [0, 2^24)";
            sum += (unsigned long long)k[t];
        }
        if (sum * QMAX + HALF >= (1ull << 32)) return "a row's accumulator could wrap (sum(k) * 1020 + 2^21 >= 2^32)";
        return nullptr;
    }

    static void lds_rows(const H*, long long nc, int cols, long long* P, long long* HP, int* v_items) {
        *P = (6 * nc + 2 + 3) & ~3LL;
        *HP = (6LL * cols + 3) & ~3LL;
        *v_items = (3 * cols) / 2 + 2;
    }

    static void note_plan(H* p, int frames) {
        if (p->fused_fits && !p->force_general)
            snprintf(p->plan, sizeof p->plan, "resize16=k_resize16_fused<rows=%d,cols=%d>;lds=%d;frames=%d", p->fused.TH, p->fused.TW, p->lds_bytes, frames);
        else
            snprintf(p->plan, sizeof p->plan, "resize16=k_resize16_h+k_resize16_v;frames=%d", frames);
    }

    static int check_alignment(H* p, const void* src, size_t src_stride_bytes, const void* dst, size_t dst_stride_bytes) {
        if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | src_stride_bytes | dst_stride_bytes) & 1u)
            return fail(p, CRTFX_E_INVALID, "frame bases and strides must be even (16-bit elements)");
        return CRTFX_OK;
    }

    static void launch(H* p, bool fused, const unsigned char* src_bytes, size_t src_stride_bytes, unsigned char* dst_bytes, size_t dst_stride_bytes, int g,
                       hipStream_t st) {
        const uint16_t* src = reinterpret_cast<const uint16_t*>(src_bytes);
        uint16_t* dst = reinterpret_cast<uint16_t*>(dst_bytes);
        uint16_t* scratch = static_cast<uint16_t*>(p->scratch);
        const size_t ss = src_stride_bytes / 2, ds = dst_stride_bytes / 2;           // the kernels' strides are in 16-bit elements
        if (fused) {
            Args a = p->fused;
            a.x = p->x; a.y = p->y;
            a.src = src; a.src_stride = ss;
            a.dst = dst; a.dst_stride = ds;
            dim3 grid((p->dw + a.TW - 1) / a.TW, (p->dh + a.TH - 1) / a.TH, g);
            hipLaunchKernelGGL(k_resize16_fused, grid, dim3(BLOCK), (size_t)p->lds_bytes, st, a);
        } else {
            hipLaunchKernelGGL(k_resize16_h, dim3((p->dw + BLOCK - 1) / BLOCK, p->sh, g), dim3(BLOCK), 0, st, src, ss, scratch, p->sh, p->sw, p->dw, p->x);
            hipLaunchKernelGGL(k_resize16_v, dim3((p->dw * 3 + BLOCK - 1) / BLOCK, p->dh, g), dim3(BLOCK), 0, st, scratch, dst, ds, p->sh, p->dw, p->y);
        }
    }
};

}  // namespace

extern "C" {

const char* crtfx_resize16_last_error(const crtfx_resize16* p) { return p ? p->err.c_str() : crtfx_resize::create_err<crtfx_resize16>().c_str(); }

int crtfx_resize16_create(int device, int src_h, int src_w, int dst_h, int dst_w, int pix_fmt,
                          const int32_t* x_min, const int32_t* x_count, const int32_t* x_k, int x_ksize,
                          const int32_t* y_min, const int32_t* y_count, const int32_t* y_k, int y_ksize, crtfx_resize16** out_plan) {
    return crtfx_resize::create<Unit>(device, src_h, src_w, dst_h, dst_w, pix_fmt, x_min, x_count, x_k, x_ksize, y_min, y_count, y_k, y_ksize, out_plan);
}

int crtfx_resize16_destroy(crtfx_resize16* p) { return crtfx_resize::destroy(p); }

int crtfx_resize16_set_option(crtfx_resize16* p, int option, int value) { return crtfx_resize::set_option<Unit>(p, option, value); }

int crtfx_resize16_last_plan(crtfx_resize16* p, char* buf, size_t n) { return crtfx_resize::last_plan(p, buf, n); }

int crtfx_resize16_run(crtfx_resize16* p, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream) {
    return crtfx_resize::run<Unit>(p, src_base, src_stride_bytes, dst_base, dst_stride_bytes, n, stream);
}

}  // extern "C"
