// crtfx_ingest.hip — the ingest stage of libcrtfx.so (include/crtfx_ingest.h): Pillow's 8-bit BILINEAR resize of uint8 RGB
// frames on the device.  A translation unit of its own: it shares no kernel, table or handle with the effect chain.  Here are its kernels,
// its handle and what the resize stages' host skeleton (crtfx_resize_host.h, host templates only) asks of a unit; create, run and the
// other entry points are that skeleton's.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "crtfx_ingest.h"
#include "crtfx_resize_host.h"

namespace crtfx_ingest_impl {

constexpr int BLOCK = 256;
constexpr int PREC = 22;                       // Pillow's PRECISION_BITS (32 - 8 - 2)
constexpr unsigned HALF = 1u << (PREC - 1);

struct Axis { const int32_t* min; const int32_t* count; const int32_t* k; int ksize; };

struct Args {
    const uint8_t* src; size_t src_stride;
    uint8_t* dst; size_t dst_stride;
    int sh, sw, dh, dw;
    Axis x, y;
    int TH, TW;                // output rows / columns per tile
    int P, HP;                 // LDS bytes per staged source row / per row of the horizontal result (multiples of 4)
    int nr_max;                // source rows of the tallest tile
    int sh_stage, sh_h, sh_v;  // log2 of the work items per row of the three phases (power-of-two rows: item -> (row, column) is a shift and a mask)
};

__device__ __forceinline__ unsigned clamp8(unsigned acc) { unsigned v = acc >> PREC; return v > 255u ? 255u : v; }

// One block = TH output rows x TW output columns of one frame.
//   phase 0  the tile's slice of the six tables -> LDS
//   phase 1  the source rows / columns its taps reach -> LDS, as aligned dwords (a row keeps its global address modulo 4, so a
//            dword in LDS is a dword in memory; only a dword that sticks out of the frame's own bytes is assembled from byte loads)
//   phase 2  horizontal pass, one thread per (source row, output pixel): three 24-bit multiply-adds per tap, uint8 result -> LDS
//   phase 3  vertical pass, one thread per ALIGNED dword of an output row (the bytes in front of the first and behind the last
//            aligned dword of the tile's row segment are single-byte items): per tap two LDS dwords funnel-shifted to the row's phase
__global__ __launch_bounds__(BLOCK) void k_ingest_fused(Args a) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int tid = threadIdx.x;
    const int ox0 = blockIdx.x * a.TW, oy0 = blockIdx.y * a.TH;
    const int ow = min(a.TW, a.dw - ox0), oh = min(a.TH, a.dh - oy0);
    const uint8_t* fsrc = a.src + (size_t)blockIdx.z * a.src_stride;
    const uint8_t* fend = fsrc + (size_t)a.sh * a.sw * 3;
    uint8_t* fdst = a.dst + (size_t)blockIdx.z * a.dst_stride;

    int* s_xmin = reinterpret_cast<int*>(lds);
    int* s_xcnt = s_xmin + a.TW;
    int* s_kx = s_xcnt + a.TW;
    int* s_ymin = s_kx + a.TW * a.x.ksize;
    int* s_ycnt = s_ymin + a.TH;
    int* s_ky = s_ycnt + a.TH;
    unsigned* S = reinterpret_cast<unsigned*>(s_ky + a.TH * a.y.ksize);
    unsigned* Hb = S + (size_t)a.nr_max * (a.P >> 2);

    // min and min + count are non-decreasing (checked by crtfx_ingest_create): the tile's source window is first tap .. last tap
    const int sx0 = a.x.min[ox0], sx1 = a.x.min[ox0 + ow - 1] + a.x.count[ox0 + ow - 1];
    const int sy0 = a.y.min[oy0], sy1 = a.y.min[oy0 + oh - 1] + a.y.count[oy0 + oh - 1];
    const int nr = sy1 - sy0, sb = (sx1 - sx0) * 3;

    for (int i = tid; i < ow; i += BLOCK) { s_xmin[i] = a.x.min[ox0 + i] - sx0; s_xcnt[i] = a.x.count[ox0 + i]; }
    for (int i = tid; i < ow * a.x.ksize; i += BLOCK) s_kx[i] = a.x.k[(size_t)ox0 * a.x.ksize + i];
    for (int i = tid; i < oh; i += BLOCK) { s_ymin[i] = a.y.min[oy0 + i] - sy0; s_ycnt[i] = a.y.count[oy0 + i]; }
    for (int i = tid; i < oh * a.y.ksize; i += BLOCK) s_ky[i] = a.y.k[(size_t)oy0 * a.y.ksize + i];

    const size_t srow = (size_t)a.sw * 3;
    for (int idx = tid; idx < (nr << a.sh_stage); idx += BLOCK) {
        const int r = idx >> a.sh_stage, d = idx & ((1 << a.sh_stage) - 1);
        const uint8_t* g = fsrc + (size_t)(sy0 + r) * srow + (size_t)sx0 * 3;
        const unsigned lead = (unsigned)(reinterpret_cast<uintptr_t>(g) & 3u);
        if (d < (int)((lead + sb + 3) >> 2)) {
            const uint8_t* p = g - lead + 4 * d;
            unsigned v;
            if (p >= fsrc && p + 4 <= fend) {
                v = *reinterpret_cast<const unsigned*>(p);
            } else {
                v = 0;
                for (int e = 0; e < 4; ++e)
                    if (p + e >= fsrc && p + e < fend) v |= (unsigned)p[e] << (8 * e);
            }
            S[r * (a.P >> 2) + d] = v;
        }
    }
    __syncthreads();

    const unsigned char* Sb = reinterpret_cast<const unsigned char*>(S);
    unsigned char* Hbb = reinterpret_cast<unsigned char*>(Hb);
    for (int idx = tid; idx < (nr << a.sh_h); idx += BLOCK) {
        const int r = idx >> a.sh_h, p = idx & ((1 << a.sh_h) - 1);
        if (p < ow) {
            const unsigned lead = (unsigned)(reinterpret_cast<uintptr_t>(fsrc + (size_t)(sy0 + r) * srow + (size_t)sx0 * 3) & 3u);
            const unsigned char* s = Sb + r * a.P + lead + s_xmin[p] * 3;
            const int* k = s_kx + p * a.x.ksize;
            const int cnt = s_xcnt[p];
            unsigned a0 = HALF, a1 = HALF, a2 = HALF;
            for (int t = 0; t < cnt; ++t) {
                const unsigned kk = (unsigned)k[t];
                a0 += __umul24(kk, s[3 * t]);
                a1 += __umul24(kk, s[3 * t + 1]);
                a2 += __umul24(kk, s[3 * t + 2]);
            }
            unsigned char* o = Hbb + r * a.HP + p * 3;
            o[0] = (unsigned char)clamp8(a0); o[1] = (unsigned char)clamp8(a1); o[2] = (unsigned char)clamp8(a2);
        }
    }
    __syncthreads();

    const int nb = ow * 3;
    const size_t drow = (size_t)a.dw * 3;
    for (int idx = tid; idx < (oh << a.sh_v); idx += BLOCK) {
        const int y = idx >> a.sh_v, i = idx & ((1 << a.sh_v) - 1);
        uint8_t* g = fdst + (size_t)(oy0 + y) * drow + (size_t)ox0 * 3;
        const int lead = min(nb, (int)((4u - (unsigned)(reinterpret_cast<uintptr_t>(g) & 3u)) & 3u));
        const int nd = (nb - lead) >> 2;
        const int* k = s_ky + y * a.y.ksize;
        const int cnt = s_ycnt[y];
        const int r0 = s_ymin[y];
        if (i < nd) {
            const int o = lead + 4 * i;                       // byte offset in the tile's row; o + 3 < nb
            const unsigned* h = Hb + r0 * (a.HP >> 2) + (o >> 2);
            const unsigned sh8 = (unsigned)(o & 3) * 8u;
            unsigned a0 = HALF, a1 = HALF, a2 = HALF, a3 = HALF;
            for (int t = 0; t < cnt; ++t) {
                const unsigned kk = (unsigned)k[t];
                unsigned v = h[0];
                if (sh8) v = (v >> sh8) | (h[1] << (32u - sh8));   // h[1] lies inside the row's pitch (HP = round4(3 * TW) + 4)
                a0 += __umul24(kk, v & 255u);
                a1 += __umul24(kk, (v >> 8) & 255u);
                a2 += __umul24(kk, (v >> 16) & 255u);
                a3 += __umul24(kk, v >> 24);
                h += a.HP >> 2;
            }
            *reinterpret_cast<unsigned*>(g + o) = clamp8(a0) | (clamp8(a1) << 8) | (clamp8(a2) << 16) | (clamp8(a3) << 24);
        } else if (i < nd + (nb - 4 * nd)) {
            const int e = i - nd;
            const int o = e < lead ? e : 4 * nd + e;           // the head bytes, then the tail behind the last aligned dword
            const unsigned char* h = Hbb + r0 * a.HP + o;
            unsigned acc = HALF;
            for (int t = 0; t < cnt; ++t) { acc += __umul24((unsigned)k[t], h[0]); h += a.HP; }
            g[o] = (uint8_t)clamp8(acc);
        }
    }
}

// General path, any tap count.  Horizontal pass: one thread per output pixel of a source row, taps read from memory.
__global__ __launch_bounds__(BLOCK) void k_ingest_h(const uint8_t* src, size_t src_stride, uint8_t* tmp, int sh, int sw, int dw, Axis x) {
    const int px = blockIdx.x * BLOCK + threadIdx.x;
    if (px >= dw) return;
    const uint8_t* s = src + (size_t)blockIdx.z * src_stride + ((size_t)blockIdx.y * sw + x.min[px]) * 3;
    const int32_t* k = x.k + (size_t)px * x.ksize;
    const int cnt = x.count[px];
    unsigned a0 = HALF, a1 = HALF, a2 = HALF;
    for (int t = 0; t < cnt; ++t) {
        const unsigned kk = (unsigned)k[t];
        a0 += __umul24(kk, s[3 * t]);
        a1 += __umul24(kk, s[3 * t + 1]);
        a2 += __umul24(kk, s[3 * t + 2]);
    }
    uint8_t* o = tmp + (((size_t)blockIdx.z * sh + blockIdx.y) * dw + px) * 3;
    o[0] = (uint8_t)clamp8(a0); o[1] = (uint8_t)clamp8(a1); o[2] = (uint8_t)clamp8(a2);
}

// Vertical pass: one thread per output byte of an output row (consecutive lanes, consecutive bytes).
__global__ __launch_bounds__(BLOCK) void k_ingest_v(const uint8_t* tmp, uint8_t* dst, size_t dst_stride, int sh, int dw, Axis y) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    const size_t row = (size_t)dw * 3;
    if ((size_t)j >= row) return;
    const int oy = blockIdx.y;
    const uint8_t* s = tmp + ((size_t)blockIdx.z * sh + y.min[oy]) * row + j;
    const int32_t* k = y.k + (size_t)oy * y.ksize;
    const int cnt = y.count[oy];
    unsigned acc = HALF;
    for (int t = 0; t < cnt; ++t) { acc += __umul24((unsigned)k[t], s[0]); s += row; }
    dst[(size_t)blockIdx.z * dst_stride + (size_t)oy * row + j] = (uint8_t)clamp8(acc);
}

}  // namespace crtfx_ingest_impl

using namespace crtfx_ingest_impl;

struct crtfx_ingest : crtfx_resize::Plan<Axis, Args> {};

namespace {

using crtfx_resize::fail;

// what crtfx_resize_host.h asks of a unit
struct Unit {
    using H = crtfx_ingest;
    static constexpr int force_option = CRTFX_INGEST_OPT_FORCE_GENERAL;
    static const char* name() { return "ingest"; }
    static int bps(int) { return 1; }

    static int check_pix_fmt(int pix_fmt) {
        if (pix_fmt == CRTFX_PIX_F16) return fail<H>(nullptr, CRTFX_E_UNSUPPORTED, "only uint8 RGB frames are resized (Pillow has no half image)");
        if (pix_fmt != CRTFX_PIX_U8) return fail<H>(nullptr, CRTFX_E_INVALID, "unknown pixel format %d", pix_fmt);
        return CRTFX_OK;
    }

    static const char* check_row(const int32_t* k, int cnt) {
        for (int t = 0; t < cnt; ++t)
            if (k[t] < 0 || k[t] >= (1 << 24)) return "a coefficient is outside [0, 2^24)";
        return nullptr;
    }

    static void lds_rows(const H*, long long nc, int cols, long long* P, long long* HP, int* v_items) {
        *P = (3 * nc + 3 + 3) & ~3LL;
        *HP = ((3LL * cols + 3) & ~3LL) + 4;
        *v_items = (3 * cols) / 4 + 6;
    }

    static void note_plan(H* p, int frames) {
        if (p->fused_fits && !p->force_general)
            snprintf(p->plan, sizeof p->plan, "ingest=k_ingest_fused<rows=%d,cols=%d>;lds=%d;frames=%d", p->fused.TH, p->fused.TW, p->lds_bytes, frames);
        else
            snprintf(p->plan, sizeof p->plan, "ingest=k_ingest_h+k_ingest_v;frames=%d", frames);
    }

    static int check_alignment(H*, const void*, size_t, const void*, size_t) { return CRTFX_OK; }

    static void launch(H* p, bool fused, const uint8_t* src, size_t ss, uint8_t* dst, size_t ds, int g, hipStream_t st) {
        uint8_t* scratch = static_cast<uint8_t*>(p->scratch);
        if (fused) {
            Args a = p->fused;
            a.x = p->x; a.y = p->y;
            a.src = src; a.src_stride = ss;
            a.dst = dst; a.dst_stride = ds;
            dim3 grid((p->dw + a.TW - 1) / a.TW, (p->dh + a.TH - 1) / a.TH, g);
            hipLaunchKernelGGL(k_ingest_fused, grid, dim3(BLOCK), (size_t)p->lds_bytes, st, a);
        } else {
            hipLaunchKernelGGL(k_ingest_h, dim3((p->dw + BLOCK - 1) / BLOCK, p->sh, g), dim3(BLOCK), 0, st, src, ss, scratch, p->sh, p->sw, p->dw, p->x);
            hipLaunchKernelGGL(k_ingest_v, dim3((p->dw * 3 + BLOCK - 1) / BLOCK, p->dh, g), dim3(BLOCK), 0, st, scratch, dst, ds, p->sh, p->dw, p->y);
        }
    }
};

}  // namespace

extern "C" {

const char* crtfx_ingest_last_error(const crtfx_ingest* p) { return p ? p->err.c_str() : crtfx_resize::create_err<crtfx_ingest>().c_str(); }

int crtfx_ingest_create(int device, int src_h, int src_w, int dst_h, int dst_w, int pix_fmt,
                        const int32_t* x_min, const int32_t* x_count, const int32_t* x_k, int x_ksize,
                        const int32_t* y_min, const int32_t* y_count, const int32_t* y_k, int y_ksize, crtfx_ingest** out_plan) {
    return crtfx_resize::create<Unit>(device, src_h, src_w, dst_h, dst_w, pix_fmt, x_min, x_count, x_k, x_ksize, y_min, y_count, y_k, y_ksize, out_plan);
}

int crtfx_ingest_destroy(crtfx_ingest* p) { return crtfx_resize::destroy(p); }

int crtfx_ingest_set_option(crtfx_ingest* p, int option, int value) { return crtfx_resize::set_option<Unit>(p, option, value); }

int crtfx_ingest_last_plan(crtfx_ingest* p, char* buf, size_t n) { return crtfx_resize::last_plan(p, buf, n); }

int crtfx_ingest_run(crtfx_ingest* p, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream) {
    return crtfx_resize::run<Unit>(p, src_base, src_stride_bytes, dst_base, dst_stride_bytes, n, stream);
}

}  // extern "C"
