// crtfx_frame_host.h — the host skeleton of the frame stages (crtfx_canvas.hip, crtfx_depth.hip, crtfx_deint.hip, crtfx_adeint.hip,
// crtfx_lut3d.hip, crtfx_interlace.hip, crtfx_signal.hip, crtfx_pal.hip): RGB frames in HBM to RGB frames in HBM, and what surrounds their kernels and does not depend on what the kernels do.
// Host code only, and everything here is a template or sits in an unnamed namespace, so every translation unit that includes it gets a
// copy of its own: the units still share no state.  The device guard and the error helpers are those of the format stages
// (crtfx_stage_host.h).  Unlike the format and resize stages these answer n == 0 with CRTFX_OK and look at no pointer then.
//
// A unit brings its kernels and its Args (kernel parameter types: they stay in the unit's own namespace; every Args has src, dst,
// src_stride, dst_stride), its handle `struct crtfx_<family> : crtfx_frames::Plan { ... }` (a handle that owns device memory frees it in
// its destructor: the handle is deleted with its device current) and a structure `U : crtfx_frames::Unit` of static members that the
// templates below take as a parameter, so that every call is a direct one:
//     using H = crtfx_<family>;
//     static constexpr int force_option;                            the number of *_OPT_FORCE_GENERAL
//     static constexpr const char* name;                            the family as the messages spell it
//     static bool vec_fits(const H*, const Batch&);                 the vec kernels' conditions
//     static void note_plan(H*, bool fits, int frames);             writes p->plan
//     static Args make_args(const H*, bool fits, const Batch&);     the launch constants of a run but for src and dst
//     static void launch(const H*, bool fits, Args&, int f, unsigned g, hipStream_t);
//                                                                   g source frames from frame f of the batch on: a.src and a.dst are theirs
// and, where the defaults of Unit do not hold, one_size and group.
#pragma once

#include "crtfx_stage_host.h"

namespace crtfx_frames {
namespace {

using crtfx_stage::DeviceGuard;
using crtfx_stage::begin_create;
using crtfx_stage::create_err;
using crtfx_stage::fail;

// what the handles share
struct Plan {
    int device = 0;
    size_t src_bytes = 0, dst_bytes = 0;       // of one frame
    int src_bps = 1, dst_bps = 1;               // bytes per sample
    int frames_out = 1;                         // output frames per source frame ...
    int frames_in = 1;                          // ... or rather per frames_in source frames: n frames give ceil(n / frames_in) * frames_out
    bool force_general = false;
    char plan[128] = "";
    std::string err;
};

// the frames of one run; prev is the frame in front of src's first, for the stage that reads one (null: none)
struct Batch {
    const void* prev;
    const void* src;
    size_t src_stride;                          // bytes
    void* dst;
    size_t dst_stride;                          // bytes, per OUTPUT frame
    int n;                                      // source frames
};

struct Unit {
    static constexpr bool one_size = false;     // source and output frames have one size, and the stride message names it once
    template <class A> static int group(const A&) { return 32768; }    // source frames per launch (grid.z); a multiple of the plan's frames_in
};

// ---- create: begin_create, the unit's own argument checks (check_size among them), then new_plan with what fills the handle ----

template <class H>
int check_size(const char* name, int v) {
    if (v < 1 || v > 32767) return fail<H>(nullptr, CRTFX_E_INVALID, "%s = %d outside 1..32767", name, v);
    return CRTFX_OK;
}

// fill(p) sets the unit's fields with the plan's device current and returns CRTFX_OK, or its own refusal (through fail<H>(nullptr, ...))
template <class U, class Fill>
int new_plan(int device, typename U::H** out_plan, Fill fill) {
    using H = typename U::H;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail<H>(nullptr, CRTFX_E_HIP, "no HIP device %d", device);
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return fail<H>(nullptr, CRTFX_E_HIP, "hipSetDevice(%d): %s", device, hipGetErrorString(guard.err));
    H* p = new (std::nothrow) H();
    if (!p) return fail<H>(nullptr, CRTFX_E_NOMEM, "out of host memory");
    p->device = device;
    if (const int rc = fill(p)) { delete p; return rc; }
    U::note_plan(p, U::vec_fits(p, Batch{nullptr, nullptr, 0, nullptr, 0, 1}), 0);
    *out_plan = p;
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

// the one option the stages share; a unit with more options keeps an entry point of its own
template <class U>
int set_option(typename U::H* p, int option, int value) {
    if (!p) return CRTFX_E_INVALID;
    if (option != U::force_option) return fail(p, CRTFX_E_INVALID, "unknown %s option %d", U::name, option);
    if (value != 0 && value != 1) return fail(p, CRTFX_E_INVALID, "FORCE_GENERAL takes 0 or 1, got %d", value);
    p->force_general = value != 0;
    U::note_plan(p, U::vec_fits(p, Batch{nullptr, nullptr, 0, nullptr, 0, 1}), 0);
    return CRTFX_OK;
}

template <class H>
int last_plan(const H* p, char* buf, size_t n) {
    if (!p || !buf || n == 0) return CRTFX_E_INVALID;
    snprintf(buf, n, "%s", p->plan);
    return CRTFX_OK;
}

template <class U>
int run(typename U::H* p, const Batch& b, void* stream) {
    if (!p) return CRTFX_E_INVALID;
    const int n = b.n;
    if (n < 0) return fail(p, CRTFX_E_INVALID, "n = %d frames", n);
    if (n == 0) { U::note_plan(p, U::vec_fits(p, b), 0); return CRTFX_OK; }
    if (!b.src || !b.dst) return fail(p, CRTFX_E_INVALID, "null frame pointer");
    const size_t n_out = ((size_t)n + p->frames_in - 1) / p->frames_in * p->frames_out;
    const uintptr_t sb = reinterpret_cast<uintptr_t>(b.src), db = reinterpret_cast<uintptr_t>(b.dst), pb = reinterpret_cast<uintptr_t>(b.prev);
    if ((p->src_bps == 2 && ((sb & 1u) || (n > 1 && (b.src_stride & 1u)))) || (p->dst_bps == 2 && ((db & 1u) || (n_out > 1 && (b.dst_stride & 1u)))))
        return fail(p, CRTFX_E_INVALID, "half frames need even bases and strides");
    if (p->src_bps == 2 && (pb & 1u)) return fail(p, CRTFX_E_INVALID, "half frames need an even prev_frame");
    if ((n > 1 && b.src_stride < p->src_bytes) || (n_out > 1 && b.dst_stride < p->dst_bytes)) {
        if (U::one_size) return fail(p, CRTFX_E_INVALID, "frame strides %zu / %zu bytes are smaller than a frame (%zu)", b.src_stride, b.dst_stride, p->src_bytes);
        return fail(p, CRTFX_E_INVALID, "frame strides %zu / %zu bytes are smaller than a frame (%zu / %zu)", b.src_stride, b.dst_stride, p->src_bytes, p->dst_bytes);
    }
    const uintptr_t se = sb + (size_t)(n - 1) * b.src_stride + p->src_bytes, de = db + (n_out - 1) * b.dst_stride + p->dst_bytes;
    if (sb < de && db < se) return fail(p, CRTFX_E_INVALID, "source and destination overlap");
    if (b.prev && pb < de && db < pb + p->src_bytes) return fail(p, CRTFX_E_INVALID, "prev_frame and destination overlap");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return fail(p, CRTFX_E_HIP, "hipGetDevice failed");
    if (dev != p->device) return fail(p, CRTFX_E_INVALID, "current device %d is not the plan's device %d (call hipSetDevice first)", dev, p->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool fits = U::vec_fits(p, b);
    auto a = U::make_args(p, fits, b);
    a.src_stride = b.src_stride; a.dst_stride = b.dst_stride;
    const int group = U::group(a);
    for (int f = 0; f < n; f += group) {
        a.src = static_cast<const uint8_t*>(b.src) + (size_t)f * b.src_stride;
        a.dst = static_cast<uint8_t*>(b.dst) + (size_t)f / p->frames_in * p->frames_out * b.dst_stride;
        U::launch(p, fits, a, f, (unsigned)(n - f < group ? n - f : group), st);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(p, CRTFX_E_HIP, "%s launch: %s", U::name, hipGetErrorString(e));
    }
    U::note_plan(p, fits, n);
    return CRTFX_OK;
}

}  // namespace
}  // namespace crtfx_frames
