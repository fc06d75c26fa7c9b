// crtfx_resize_host.h — the host skeleton of the resize stages (crtfx_ingest.hip, crtfx_resize16.hip, crtfx_resample.hip): what surrounds their
// kernels and does not depend on the sample type or the filter.  Host code only, and everything here is a template or sits in an unnamed
// namespace, so every translation unit that includes it gets a copy of its own: the units still share no state.  The device guard and the
// error helpers are those of the format stages (crtfx_stage_host.h).
//
// A unit brings its kernels, its Axis and Args (kernel parameter types: they stay in the unit's own namespace), its handle
// `struct crtfx_<family> : crtfx_resize::Plan<Axis, Args> {}` and a structure U of static members that the templates below take as a
// parameter, so that every call is a direct one:
//     using H = crtfx_<family>;
//     static constexpr int force_option;                            the number of *_OPT_FORCE_GENERAL
//     static const char* name();                                    the family as the messages spell it
//     static int check_pix_fmt(int pix_fmt);                        CRTFX_OK, or the unit's own refusal (through fail<H>)
//     static int bps(int pix_fmt);                                  bytes per sample
//     static const char* check_row(const int32_t* k, int count);    the coefficient rule of one table row: nullptr, or what it breaks
//     static void lds_rows(const H*, long long nc, int cols, long long* P, long long* HP, int* v_items);
//                                                                   LDS bytes per staged source row of nc pixels / per row of the horizontal
//                                                                   result of cols pixels; work items of one output row in the vertical phase
//     static void note_plan(H*, int frames);                        writes p->plan
//     static int check_alignment(H*, src, src_stride, dst, dst_stride);  CRTFX_OK, or the unit's own refusal (through fail)
//     static void launch(H*, bool fused, const unsigned char* src, size_t src_stride_bytes, unsigned char* dst, size_t dst_stride_bytes,
//                        int g, hipStream_t);                       g frames: the fused kernel, or the horizontal and the vertical pass
#pragma once

#include <vector>

#include "crtfx_stage_host.h"

namespace crtfx_resize {
namespace {

using crtfx_stage::DeviceGuard;
using crtfx_stage::create_err;
using crtfx_stage::fail;

constexpr int LDS_BUDGET = 40960;              // four blocks per CU (160 KB of LDS)
constexpr size_t SCRATCH_BYTES = 64u << 20;    // general path: frames per group = what fits this much horizontal-pass scratch (at least one, at most 64)

// what the handles share
template <class Axis, class Args>
struct Plan {
    int device = 0;
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
    char plan[160] = "";
    std::string err;
};

inline int log2_ceil(int v) { int s = 0; while ((1 << s) < v) ++s; return s; }

// the rules crtfx_ingest.h states for a table, and the unit's rule for the coefficients of a row; the kernels' bounds rest on them
template <class U>
const char* check_axis(const int32_t* mn, const int32_t* cnt, const int32_t* k, int ksize, int n_in, int n_out) {
    for (int i = 0; i < n_out; ++i) {
        if (mn[i] < 0 || cnt[i] < 1 || cnt[i] > ksize || mn[i] > n_in - cnt[i]) return "a tap window leaves the source (min >= 0, 1 <= count <= ksize, min + count <= n_in)";
        if (i && (mn[i] < mn[i - 1] || mn[i] + cnt[i] < mn[i - 1] + cnt[i - 1])) return "min and min + count must be non-decreasing";
        if (const char* why = U::check_row(k + (size_t)i * ksize, cnt[i])) return why;
    }
    return nullptr;
}

// largest source extent (taps of the first .. last output index) over the tiles of `tile` output indices
inline int max_extent(const int32_t* mn, const int32_t* cnt, int n_out, int tile) {
    int m = 0;
    for (int o = 0; o < n_out; o += tile) {
        const int last = (o + tile < n_out ? o + tile : n_out) - 1;
        const int e = mn[last] + cnt[last] - mn[o];
        if (e > m) m = e;
    }
    return m;
}

// the first tile shape whose tables, staged source rows and horizontal result meet the LDS budget
template <class U>
void plan_fused(typename U::H* p, const int32_t* xmin, const int32_t* xcnt, const int32_t* ymin, const int32_t* ycnt) {
    static const int shapes[][2] = {{32, 128}, {32, 64}, {16, 128}, {16, 64}, {8, 64}, {8, 32}, {4, 32}};
    for (const auto& s : shapes) {
        const int TH = s[0], TW = s[1];
        const int rows = TH < p->dh ? TH : p->dh, cols = TW < p->dw ? TW : p->dw;
        const long long nr = max_extent(ymin, ycnt, p->dh, TH), nc = max_extent(xmin, xcnt, p->dw, TW);
        long long P = 0, HP = 0;
        int v_items = 0;
        U::lds_rows(p, nc, cols, &P, &HP, &v_items);
        const long long tab = 4LL * (2 * cols + (long long)cols * p->x.ksize + 2 * rows + (long long)rows * p->y.ksize);
        const long long total = tab + nr * (P + HP);
        if (total > LDS_BUDGET) continue;
        auto& a = p->fused;
        a = {};
        a.sh = p->sh; a.sw = p->sw; a.dh = p->dh; a.dw = p->dw;
        a.TH = rows; a.TW = cols; a.P = (int)P; a.HP = (int)HP; a.nr_max = (int)nr;
        a.sh_stage = log2_ceil((int)(P >> 2));
        a.sh_h = log2_ceil(cols);
        a.sh_v = log2_ceil(v_items);
        p->lds_bytes = (int)total;
        p->fused_fits = true;
        return;
    }
}

template <class U>
int create(int device, int src_h, int src_w, int dst_h, int dst_w, int pix_fmt,
           const int32_t* x_min, const int32_t* x_count, const int32_t* x_k, int x_ksize,
           const int32_t* y_min, const int32_t* y_count, const int32_t* y_k, int y_ksize, typename U::H** out_plan) {
    using H = typename U::H;
    create_err<H>().clear();
    if (!out_plan) return fail<H>(nullptr, CRTFX_E_INVALID, "out_plan is null");
    *out_plan = nullptr;
    if (const int rc = U::check_pix_fmt(pix_fmt)) return rc;
    if (src_h < 1 || src_w < 1 || dst_h < 1 || dst_w < 1 || src_h > 32767 || src_w > 32767 || dst_h > 32767 || dst_w > 32767)
        return fail<H>(nullptr, CRTFX_E_INVALID, "sizes %dx%d -> %dx%d outside 1..32767", src_h, src_w, dst_h, dst_w);
    if (!x_min || !x_count || !x_k || !y_min || !y_count || !y_k) return fail<H>(nullptr, CRTFX_E_INVALID, "a table is null");
    if (x_ksize < 1 || y_ksize < 1) return fail<H>(nullptr, CRTFX_E_INVALID, "ksize %d / %d < 1", x_ksize, y_ksize);
    if (const char* why = check_axis<U>(x_min, x_count, x_k, x_ksize, src_w, dst_w)) return fail<H>(nullptr, CRTFX_E_INVALID, "x tables: %s", why);
    if (const char* why = check_axis<U>(y_min, y_count, y_k, y_ksize, src_h, dst_h)) return fail<H>(nullptr, CRTFX_E_INVALID, "y tables: %s", why);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail<H>(nullptr, CRTFX_E_HIP, "no HIP device %d", device);
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return fail<H>(nullptr, CRTFX_E_HIP, "hipSetDevice(%d): %s", device, hipGetErrorString(guard.err));
    H* p = new (std::nothrow) H();
    if (!p) return fail<H>(nullptr, CRTFX_E_NOMEM, "out of host memory");
    p->device = device; p->bps = U::bps(pix_fmt);
    p->sh = src_h; p->sw = src_w; p->dh = dst_h; p->dw = dst_w;
    p->x.ksize = x_ksize; p->y.ksize = y_ksize;
    plan_fused<U>(p, x_min, x_count, y_min, y_count);

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
        fail<H>(nullptr, code, "crtfx_%s_create: %s", U::name(), hipGetErrorString(e));
        if (p->tables) (void)hipFree(p->tables);
        if (p->scratch) (void)hipFree(p->scratch);
        delete p;
        return code;
    }
    int32_t* t = p->tables;
    p->x.min = t; t += dst_w; p->x.count = t; t += dst_w; p->x.k = t; t += (size_t)dst_w * x_ksize; p->x.ksize = x_ksize;
    p->y.min = t; t += dst_h; p->y.count = t; t += dst_h; p->y.k = t; p->y.ksize = y_ksize;
    U::note_plan(p, 0);
    *out_plan = p;
    return CRTFX_OK;
}

template <class H>
int destroy(H* p) {
    if (!p) return CRTFX_OK;
    DeviceGuard guard(p->device);
    (void)hipDeviceSynchronize();
    if (p->tables) (void)hipFree(p->tables);
    if (p->scratch) (void)hipFree(p->scratch);
    delete p;
    return CRTFX_OK;
}

// the one option the three stages share; a unit with more options keeps an entry point of its own
template <class U>
int set_option(typename U::H* p, int option, int value) {
    if (!p) return CRTFX_E_INVALID;
    if (option != U::force_option) return fail(p, CRTFX_E_INVALID, "unknown %s option %d", U::name(), option);
    if (value != 0 && value != 1) return fail(p, CRTFX_E_INVALID, "FORCE_GENERAL takes 0 or 1, got %d", value);
    p->force_general = value != 0;
    U::note_plan(p, 0);
    return CRTFX_OK;
}

template <class H>
int last_plan(const H* p, char* buf, size_t n) {
    if (!p || !buf || n == 0) return CRTFX_E_INVALID;
    snprintf(buf, n, "%s", p->plan);
    return CRTFX_OK;
}

template <class U>
int run(typename U::H* p, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream) {
    if (!p) return CRTFX_E_INVALID;
    if (!src_base || !dst_base) return fail(p, CRTFX_E_INVALID, "null frame pointer");
    if (n < 1) return fail(p, CRTFX_E_INVALID, "n = %d frames", n);
    if (const int rc = U::check_alignment(p, src_base, src_stride_bytes, dst_base, dst_stride_bytes)) return rc;
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
        U::launch(p, fused, src + (size_t)f * src_stride_bytes, src_stride_bytes, dst + (size_t)f * dst_stride_bytes, dst_stride_bytes, g, st);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(p, CRTFX_E_HIP, "%s launch: %s", U::name(), hipGetErrorString(e));
    }
    U::note_plan(p, n);
    return CRTFX_OK;
}

}  // namespace
}  // namespace crtfx_resize
