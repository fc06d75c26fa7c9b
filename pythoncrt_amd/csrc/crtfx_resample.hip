// crtfx_resample.hip — the filtered resampler of libcrtfx.so (include/crtfx_resample.h): Pillow's 8-bit two-pass resize with signed taps (BOX,
// BILINEAR, HAMMING, BICUBIC, LANCZOS), h x w x 3 RGB frames of uint8 or of halves on the quarter-code scale, on the device.  A translation
// unit of its own: it shares no kernel, table or handle with the effect chain or with the two BILINEAR stages whose structure it follows; of
// the format stages' host skeleton (crtfx_stage_host.h, host templates only) it takes the device guard and the error helper.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "crtfx_resample.h"
#include "crtfx_stage_host.h"

namespace crtfx_resample_impl {

constexpr int BLOCK = 256;
constexpr int PREC = 22;                       // Pillow's PRECISION_BITS (32 - 8 - 2)
constexpr int HALF = 1 << (PREC - 1);
constexpr int LDS_BUDGET = 40960;              // four blocks per CU (160 KB of LDS)
constexpr size_t SCRATCH_BYTES = 64u << 20;    // general path: frames per group = what fits this much horizontal-pass scratch (at least one, at most 64)

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
using namespace crtfx_stage;       // DeviceGuard, fail and create_err; the plan, create and run are this stage's own

struct crtfx_resample {
    int device = 0;
    int pix_fmt = CRTFX_PIX_U8;
    int bps = 1;                        // bytes per sample
    int sh = 0, sw = 0, dh = 0, dw = 0;
    int32_t* tables = nullptr;          // one device allocation: x min | x count | x k | y min | y count | y k
    Axis x{}, y{};
    bool fused_fits = false;            // some tile shape meets the LDS budget
    Args fused{};                       // its launch constants (frame pointers filled per run)
    int lds_bytes = 0;
    void* scratch = nullptr;            // general path: scratch_frames x sh x dw x 3 samples
    int scratch_frames = 0;
    bool force_general = false;
    bool acc64 = false;
    char plan[160] = "";
    std::string err;
};

namespace {

int log2_ceil(int v) { int s = 0; while ((1 << s) < v) ++s; return s; }

// the rules crtfx_resample.h states for a table; the kernels' bounds and the accumulators' ranges rest on them
const char* check_axis(const int32_t* mn, const int32_t* cnt, const int32_t* k, int ksize, int n_in, int n_out) {
    for (int i = 0; i < n_out; ++i) {
        if (mn[i] < 0 || cnt[i] < 1 || cnt[i] > ksize || mn[i] > n_in - cnt[i]) return "a tap window leaves the source (min >= 0, 1 <= count <= ksize, min + count <= n_in)";
        if (i && (mn[i] < mn[i - 1] || mn[i] + cnt[i] < mn[i - 1] + cnt[i - 1])) return "min and min + count must be non-decreasing";
        long long pos = 0, neg = 0;
        for (int t = 0; t < cnt[i]; ++t) {
            const int32_t kk = k[(size_t)i * ksize + t];
            if (kk < -(1 << 23) || kk >= (1 << 23)) return "a coefficient is outside [-2^23, 2^23)";
            if (kk > 0) pos += kk; else neg += kk;
        }
        if ((long long)HALF + 255 * pos >= (1LL << 31) || 255 * neg <= -(1LL << 31))
            return "a row's accumulator could leave int32 (2^21 + 255 * sum(k > 0) < 2^31 and 255 * sum(k < 0) > -2^31)";
    }
    return nullptr;
}

// largest source extent (taps of the first .. last output index) over the tiles of `tile` output indices
int max_extent(const int32_t* mn, const int32_t* cnt, int n_out, int tile) {
    int m = 0;
    for (int o = 0; o < n_out; o += tile) {
        const int last = (o + tile < n_out ? o + tile : n_out) - 1;
        const int e = mn[last] + cnt[last] - mn[o];
        if (e > m) m = e;
    }
    return m;
}

void plan_fused(crtfx_resample* p, const int32_t* xmin, const int32_t* xcnt, const int32_t* ymin, const int32_t* ycnt) {
    static const int shapes[][2] = {{32, 128}, {32, 64}, {16, 128}, {16, 64}, {8, 64}, {8, 32}, {4, 32}};
    const long long b = p->bps;
    for (const auto& s : shapes) {
        const int TH = s[0], TW = s[1];
        const int rows = TH < p->dh ? TH : p->dh, cols = TW < p->dw ? TW : p->dw;
        const long long nr = max_extent(ymin, ycnt, p->dh, TH), nc = max_extent(xmin, xcnt, p->dw, TW);
        const long long P = (3 * b * nc + 3 + 3) & ~3LL, HP = ((3 * b * cols + 3) & ~3LL) + 4;
        const long long tab = 4LL * (2 * cols + (long long)cols * p->x.ksize + 2 * rows + (long long)rows * p->y.ksize);
        const long long total = tab + nr * (P + HP);
        if (total > LDS_BUDGET) continue;
        Args& a = p->fused;
        a = Args{};
        a.sh = p->sh; a.sw = p->sw; a.dh = p->dh; a.dw = p->dw;
        a.TH = rows; a.TW = cols; a.P = (int)P; a.HP = (int)HP; a.nr_max = (int)nr;
        a.sh_stage = log2_ceil((int)(P >> 2));
        a.sh_h = log2_ceil(cols);
        a.sh_v = log2_ceil((3 * (int)b * cols) / 4 + 6);          // aligned dwords of a row segment + at most three samples on either side
        p->lds_bytes = (int)total;
        p->fused_fits = true;
        return;
    }
}

void note_plan(crtfx_resample* p, int frames) {
    const char* px = p->bps == 1 ? "u8" : "half";
    const char* acc = p->acc64 ? ";acc=i64" : "";
    if (p->fused_fits && !p->force_general)
        snprintf(p->plan, sizeof p->plan, "resample=k_resample_fused<%s,rows=%d,cols=%d>;lds=%d;frames=%d%s", px, p->fused.TH, p->fused.TW, p->lds_bytes, frames, acc);
    else
        snprintf(p->plan, sizeof p->plan, "resample=k_resample_h+k_resample_v<%s>;frames=%d%s", px, frames, acc);
}

template <typename E, typename ACC>
void launch(crtfx_resample* p, bool fused, const unsigned char* src, size_t ss, unsigned char* dst, size_t ds, int g, hipStream_t st) {
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

}  // namespace

extern "C" {

const char* crtfx_resample_last_error(const crtfx_resample* p) { return p ? p->err.c_str() : create_err<crtfx_resample>().c_str(); }

int crtfx_resample_create(int device, int src_h, int src_w, int dst_h, int dst_w, int pix_fmt,
                          const int32_t* x_min, const int32_t* x_count, const int32_t* x_k, int x_ksize,
                          const int32_t* y_min, const int32_t* y_count, const int32_t* y_k, int y_ksize, crtfx_resample** out_plan) {
    create_err<crtfx_resample>().clear();
    if (!out_plan) return fail<crtfx_resample>(nullptr, CRTFX_E_INVALID, "out_plan is null");
    *out_plan = nullptr;
    if (pix_fmt != CRTFX_PIX_U8 && pix_fmt != CRTFX_PIX_F16) return fail<crtfx_resample>(nullptr, CRTFX_E_INVALID, "unknown pixel format %d", pix_fmt);
    if (src_h < 1 || src_w < 1 || dst_h < 1 || dst_w < 1 || src_h > 32767 || src_w > 32767 || dst_h > 32767 || dst_w > 32767)
        return fail<crtfx_resample>(nullptr, CRTFX_E_INVALID, "sizes %dx%d -> %dx%d outside 1..32767", src_h, src_w, dst_h, dst_w);
    if (!x_min || !x_count || !x_k || !y_min || !y_count || !y_k) return fail<crtfx_resample>(nullptr, CRTFX_E_INVALID, "a table is null");
    if (x_ksize < 1 || y_ksize < 1) return fail<crtfx_resample>(nullptr, CRTFX_E_INVALID, "ksize %d / %d < 1", x_ksize, y_ksize);
    if (const char* why = check_axis(x_min, x_count, x_k, x_ksize, src_w, dst_w)) return fail<crtfx_resample>(nullptr, CRTFX_E_INVALID, "x tables: %s", why);
    if (const char* why = check_axis(y_min, y_count, y_k, y_ksize, src_h, dst_h)) return fail<crtfx_resample>(nullptr, CRTFX_E_INVALID, "y tables: %s", why);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail<crtfx_resample>(nullptr, CRTFX_E_HIP, "no HIP device %d", device);
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return fail<crtfx_resample>(nullptr, CRTFX_E_HIP, "hipSetDevice(%d): %s", device, hipGetErrorString(guard.err));
    crtfx_resample* p = new (std::nothrow) crtfx_resample();
    if (!p) return fail<crtfx_resample>(nullptr, CRTFX_E_NOMEM, "out of host memory");
    p->device = device; p->pix_fmt = pix_fmt; p->bps = pix_fmt == CRTFX_PIX_U8 ? 1 : 2;
    p->sh = src_h; p->sw = src_w; p->dh = dst_h; p->dw = dst_w;
    p->x.ksize = x_ksize; p->y.ksize = y_ksize;
    plan_fused(p, x_min, x_count, y_min, y_count);

    std::vector<int32_t> host;
    host.reserve((size_t)dst_w * (2 + x_ksize) + (size_t)dst_h * (2 + y_ksize));
    host.insert(host.end(), x_min, x_min + dst_w);
    host.insert(host.end(), x_count, x_count + dst_w);
    host.insert(host.end(), x_k, x_k + (size_t)dst_w * x_ksize);
    host.insert(host.end(), y_min, y_min + dst_h);
    host.insert(host.end(), y_count, y_count + dst_h);
    host.insert(host.end(), y_k, y_k + (size_t)dst_h * y_ksize);
    const size_t frame_tmp = (size_t)src_h * dst_w * 3 * p->bps;
    p->scratch_frames = p->fused_fits ? 1 : (int)(SCRATCH_BYTES / frame_tmp);      // behind a fused plan the general path is an A/B switch only
    if (p->scratch_frames < 1) p->scratch_frames = 1;
    if (p->scratch_frames > 64) p->scratch_frames = 64;
    hipError_t e = hipMalloc((void**)&p->tables, host.size() * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(&p->scratch, frame_tmp * p->scratch_frames);
    if (e == hipSuccess) e = hipMemcpy(p->tables, host.data(), host.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        const int code = e == hipErrorOutOfMemory ? CRTFX_E_NOMEM : CRTFX_E_HIP;
        fail<crtfx_resample>(nullptr, code, "crtfx_resample_create: %s", hipGetErrorString(e));
        if (p->tables) (void)hipFree(p->tables);
        if (p->scratch) (void)hipFree(p->scratch);
        delete p;
        return code;
    }
    int32_t* t = p->tables;
    p->x.min = t; t += dst_w; p->x.count = t; t += dst_w; p->x.k = t; t += (size_t)dst_w * x_ksize; p->x.ksize = x_ksize;
    p->y.min = t; t += dst_h; p->y.count = t; t += dst_h; p->y.k = t; p->y.ksize = y_ksize;
    note_plan(p, 0);
    *out_plan = p;
    return CRTFX_OK;
}

int crtfx_resample_destroy(crtfx_resample* p) {
    if (!p) return CRTFX_OK;
    DeviceGuard guard(p->device);
    (void)hipDeviceSynchronize();
    if (p->tables) (void)hipFree(p->tables);
    if (p->scratch) (void)hipFree(p->scratch);
    delete p;
    return CRTFX_OK;
}

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
    note_plan(p, 0);
    return CRTFX_OK;
}

int crtfx_resample_last_plan(crtfx_resample* p, char* buf, size_t n) {
    if (!p || !buf || n == 0) return CRTFX_E_INVALID;
    snprintf(buf, n, "%s", p->plan);
    return CRTFX_OK;
}

int crtfx_resample_run(crtfx_resample* p, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream) {
    if (!p) return CRTFX_E_INVALID;
    if (!src_base || !dst_base) return fail(p, CRTFX_E_INVALID, "null frame pointer");
    if (n < 1) return fail(p, CRTFX_E_INVALID, "n = %d frames", n);
    if (p->bps == 2 && ((reinterpret_cast<uintptr_t>(src_base) | reinterpret_cast<uintptr_t>(dst_base) | src_stride_bytes | dst_stride_bytes) & 1u))
        return fail(p, CRTFX_E_INVALID, "frame bases and strides of half frames must be even (16-bit elements)");
    const size_t src_bytes = (size_t)p->sh * p->sw * 3 * p->bps, dst_bytes = (size_t)p->dh * p->dw * 3 * p->bps;
    if (n > 1 && (src_stride_bytes < src_bytes || dst_stride_bytes < dst_bytes))
        return fail(p, CRTFX_E_INVALID, "frame strides %zu / %zu bytes are smaller than a frame (%zu / %zu)", src_stride_bytes, dst_stride_bytes, src_bytes, dst_bytes);
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return fail(p, CRTFX_E_HIP, "hipGetDevice failed");
    if (dev != p->device) return fail(p, CRTFX_E_INVALID, "current device %d is not the plan's device %d (call hipSetDevice first)", dev, p->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned char* src = static_cast<const unsigned char*>(src_base);
    unsigned char* dst = static_cast<unsigned char*>(dst_base);
    const bool fused = p->fused_fits && !p->force_general;
    const int group = fused ? 32768 : p->scratch_frames;          // grid.z; the general path's scratch
    for (int f = 0; f < n; f += group) {
        const int g = n - f < group ? n - f : group;
        const unsigned char* s = src + (size_t)f * src_stride_bytes;
        unsigned char* d = dst + (size_t)f * dst_stride_bytes;
        if (p->bps == 1) launch<uint8_t, AccU8>(p, fused, s, src_stride_bytes, d, dst_stride_bytes, g, st);
        else if (p->acc64) launch<uint16_t, Acc64>(p, fused, s, src_stride_bytes, d, dst_stride_bytes, g, st);
        else launch<uint16_t, AccAB>(p, fused, s, src_stride_bytes, d, dst_stride_bytes, g, st);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(p, CRTFX_E_HIP, "resample launch: %s", hipGetErrorString(e));
    }
    note_plan(p, n);
    return CRTFX_OK;
}

}  // extern "C"
