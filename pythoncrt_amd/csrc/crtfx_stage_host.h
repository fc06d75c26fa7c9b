// crtfx_stage_host.h — the host skeleton of the format stages (crtfx_unpack.hip, crtfx_egress.hip, crtfx_deep.hip, crtfx_422.hip,
// crtfx_444.hip, crtfx_sited.hip, crtfx_egress_sited.hip, crtfx_field420.hip, crtfx_egress_field420.hip): what surrounds their kernels and does not depend on the format.  Host code only, and everything here is a template or
// sits in an unnamed namespace, so every translation unit that includes it gets a copy of its own: the units still share no state.  The resize
// stages' skeleton (crtfx_resize_host.h: crtfx_ingest.hip, crtfx_resize16.hip, crtfx_resample.hip) takes DeviceGuard, create_err and fail from
// here and nothing else; the frame stages' skeleton (crtfx_frame_host.h: crtfx_canvas.hip, crtfx_depth.hip, crtfx_deint.hip, crtfx_adeint.hip,
// crtfx_lut3d.hip, crtfx_interlace.hip) takes those three and begin_create.
//
// A unit brings its kernels, its Args, a plan `struct Plan : StagePlan { Args args{}; }`, its handle types (the plan itself or structures
// derived from it) and a structure U of static members that the templates below take as a parameter, so that every call is a direct one:
//     static constexpr int block, force_option;                     threads per block; the number of *_OPT_FORCE_GENERAL
//     static const char* name(bool egress);                         the family as the messages and the plan string spell it
//     static void note_plan(Plan*, bool vec, int frames);           writes p->plan
//     static int check_alignment(Plan*, src, src_stride, dst, dst_stride);  CRTFX_OK, or the unit's own refusal (through fail)
//     static int items(const Args&, bool vec);                      lanes of one frame
//     static void launch(const Plan*, bool vec, dim3 grid, hipStream_t, const Args&);
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <new>
#include <string>

#include "crtfx.h"

namespace crtfx_stage {
namespace {

struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) { err = hipSetDevice(dev); switched = err == hipSuccess; }
    }
    ~DeviceGuard() { if (switched && prev >= 0) (void)hipSetDevice(prev); }
};

// what the handles share; a unit adds `Args args` (launch constants; the frame pointers are filled per run)
struct StagePlan {
    bool egress = false;
    int device = 0;
    int layout = 0;
    size_t frame_bytes = 0;             // of the format's side
    size_t rgb_bytes = 0;               // of the RGB side
    bool force_general = false;
    char plan[128] = "";
    std::string err;
};

// the error of the last failed create of handle type H on this thread: what crtfx_<family>_last_error(NULL) returns
template <class H> std::string& create_err() { thread_local std::string s; return s; }

template <class H>
int fail(H* p, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (p) p->err = buf; else create_err<H>() = buf;
    return code;
}

// source: the accumulator of one row stays inside int32 for every input, every centred sample within +-max_sample
constexpr int MATRIX_SH = 16;           // fractional bits of every stage's matrix
inline bool source_row_fits(const int32_t* row, long long max_sample) {
    long long s = 1LL << (MATRIX_SH - 1);
    for (int i = 0; i < 3; ++i) s += (row[i] < 0 ? -(long long)row[i] : (long long)row[i]) * max_sample;
    return s < (1LL << 31);
}

// egress: the accumulator of one row stays in [0, 2^31) for every input: constant + (negative entries) * X >= 0, constant + (positive entries) * X < 2^31
inline bool egress_row_fits(const int32_t* row, long long konst, long long x) {
    long long pos = 0, neg = 0;
    for (int i = 0; i < 3; ++i) { if (row[i] > 0) pos += row[i]; else neg += row[i]; }
    return konst + neg * x >= 0 && konst + pos * x < (1LL << 31);
}

template <class P>
bool vec_fits(const P* p, const void* src, size_t src_stride, const void* dst, size_t dst_stride, int n) {
    if (p->force_general || (p->args.w & 7)) return false;
    if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 3u) return false;
    return n <= 1 || !((src_stride | dst_stride) & 3u);
}

// ---- create, in the order of its checks: begin_create, the unit's refusal of the other pixel format, check_create, the unit's constants
// and their range check, new_plan, the unit's sizes ----

template <class H>
int begin_create(H** out_plan) {
    create_err<H>().clear();
    if (!out_plan) return fail<H>(nullptr, CRTFX_E_INVALID, "out_plan is null");
    *out_plan = nullptr;
    return CRTFX_OK;
}

template <class H>
int check_create(int pix_fmt, int want_pix_fmt, int h, int w, int layout, bool layout_known, const int32_t* m, const int32_t* off, int max_sample) {
    if (pix_fmt != want_pix_fmt) return fail<H>(nullptr, CRTFX_E_INVALID, "unknown pixel format %d", pix_fmt);
    if (h < 1 || w < 1 || h > 32767 || w > 32767) return fail<H>(nullptr, CRTFX_E_INVALID, "size %dx%d outside 1..32767", h, w);
    if (!layout_known) return fail<H>(nullptr, CRTFX_E_INVALID, "unknown layout %d", layout);
    if (!m || !off) return fail<H>(nullptr, CRTFX_E_INVALID, "a table is null");
    for (int i = 0; i < 3; ++i)
        if (off[i] < 0 || off[i] > max_sample) return fail<H>(nullptr, CRTFX_E_INVALID, "offset %d = %d outside 0..%d", i, off[i], max_sample);
    return CRTFX_OK;
}

// the handle, with the fields every stage fills the same way: device, layout, h, w and the matrix
template <class H>
int new_plan(bool egress, int device, int layout, int h, int w, const int32_t* m, H** out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail<H>(nullptr, CRTFX_E_HIP, "no HIP device %d", device);
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return fail<H>(nullptr, CRTFX_E_HIP, "hipSetDevice(%d): %s", device, hipGetErrorString(guard.err));
    H* p = new (std::nothrow) H();
    if (!p) return fail<H>(nullptr, CRTFX_E_NOMEM, "out of host memory");
    p->egress = egress; p->device = device; p->layout = layout;
    p->args.h = h; p->args.w = w;
    for (int i = 0; i < 9; ++i) p->args.m[i] = m[i];
    *out = p;
    return CRTFX_OK;
}

// ---- the other entry points ----

template <class H>
int destroy(H* p) {
    if (!p) return CRTFX_OK;
    DeviceGuard guard(p->device);
    (void)hipDeviceSynchronize();
    delete p;
    return CRTFX_OK;
}

template <class U, class H>
int set_option(H* p, int option, int value) {
    if (!p) return CRTFX_E_INVALID;
    if (option != U::force_option) return fail(p, CRTFX_E_INVALID, "unknown %s option %d", U::name(p->egress), option);
    if (value != 0 && value != 1) return fail(p, CRTFX_E_INVALID, "FORCE_GENERAL takes 0 or 1, got %d", value);
    p->force_general = value != 0;
    U::note_plan(p, vec_fits(p, nullptr, 0, nullptr, 0, 1), 0);
    return CRTFX_OK;
}

template <class H>
int last_plan(const H* p, char* buf, size_t n) {
    if (!p || !buf || n == 0) return CRTFX_E_INVALID;
    snprintf(buf, n, "%s", p->plan);
    return CRTFX_OK;
}

template <class U, class H>
int run_frames(H* p, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream) {
    if (!p) return CRTFX_E_INVALID;
    if (!src_base || !dst_base) return fail(p, CRTFX_E_INVALID, "null frame pointer");
    if (n < 1) return fail(p, CRTFX_E_INVALID, "n = %d frames", n);
    if (const int rc = U::check_alignment(p, src_base, src_stride_bytes, dst_base, dst_stride_bytes)) return rc;
    const size_t src_bytes = p->egress ? p->rgb_bytes : p->frame_bytes, dst_bytes = p->egress ? p->frame_bytes : p->rgb_bytes;
    if (n > 1 && (src_stride_bytes < src_bytes || dst_stride_bytes < dst_bytes))
        return fail(p, CRTFX_E_INVALID, "frame strides %zu / %zu bytes are smaller than a frame (%zu / %zu)", src_stride_bytes, dst_stride_bytes, src_bytes, dst_bytes);
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return fail(p, CRTFX_E_HIP, "hipGetDevice failed");
    if (dev != p->device) return fail(p, CRTFX_E_INVALID, "current device %d is not the plan's device %d (call hipSetDevice first)", dev, p->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint8_t* src = static_cast<const uint8_t*>(src_base);
    uint8_t* dst = static_cast<uint8_t*>(dst_base);
    const bool vec = vec_fits(p, src_base, src_stride_bytes, dst_base, dst_stride_bytes, n);
    const int items = U::items(p->args, vec);                                                // below 2^30 for every stage
    const int group = 32768;                                                                 // grid.z
    for (int f = 0; f < n; f += group) {
        auto a = p->args;
        a.src = src + (size_t)f * src_stride_bytes; a.src_stride = src_stride_bytes;
        a.dst = dst + (size_t)f * dst_stride_bytes; a.dst_stride = dst_stride_bytes;
        const dim3 grid((items + U::block - 1) / U::block, 1, n - f < group ? n - f : group);
        U::launch(p, vec, grid, st, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(p, CRTFX_E_HIP, "%s launch: %s", U::name(p->egress), hipGetErrorString(e));
    }
    U::note_plan(p, vec, n);
    return CRTFX_OK;
}

}  // namespace
}  // namespace crtfx_stage
