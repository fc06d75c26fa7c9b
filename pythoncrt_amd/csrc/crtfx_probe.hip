// crtfx_probe.hip — the source probe (include/crtfx_probe.h): one record of exact integer statistics per RGB frame — channel extremes, luma
// sum, histogram, row and column sums, and the three comb sums that tell a woven frame's field order.  A vec and a general kernel per sample
// type, the kernel that initialises the records, the host glue, the C entry points.  The sample types, the quantiser and the dword loads are
// crtfx_deint.hip's (crtfx_edge.hip.h).

#include <hip/hip_runtime.h>

#include <cstdio>
#include <type_traits>

#include "crtfx_probe.h"
#include "crtfx_edge.hip.h"
#include "crtfx_frame_host.h"

namespace crtfx_probe_impl {

using namespace crtfx_deint_impl;       // vec / general, u8 / f16, load_dwords, unpack_codes, BLOCK

// Launch constants.
struct Args {
    const uint8_t* src;
    const uint8_t* prev;                // the previous frame of source frame 0 of this launch, or null: that frame has none
    uint8_t* dst;                       // the records
    size_t src_stride, dst_stride;      // bytes
    uint32_t h, w;
    uint32_t words;                     // of one record
};

// the record's layout (crtfx_probe.h)
constexpr uint32_t W_FLAGS = 0, W_MIN = 1, W_MAX = 4, W_SUM = 8, W_CUR = 10, W_EVEN = 12, W_ODD = 14, W_HIST = 16, W_ROWS = 272;

// the tile of a block: TILE_ROWS rows, WAVE_ROWS consecutive ones per wave, x 64 lanes of PX pixels
constexpr int WAVES = BLOCK / 64, WAVE_ROWS = 8, TILE_ROWS = WAVES * WAVE_ROWS;
constexpr int COPIES = 16;              // lane-interleaved sub-histograms in LDS

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint32_t t = (uint32_t)__shfl_xor((int)v, o, 64); v = t < v ? t : v; }
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint32_t t = (uint32_t)__shfl_xor((int)v, o, 64); v = t > v ? t : v; }
    return v;
}

__device__ __forceinline__ int luma(int r, int g, int b) { return (54 * r + 183 * g + 19 * b + 128) >> 8; }

// the codes of a lane's PX pixels of one row: vec as dword multiples at a dword-aligned address, general sample by sample
template <class P, class Path, int PX>
__device__ __forceinline__ void load_codes(const uint8_t* __restrict__ row, uint32_t x, int (&q)[3 * PX]) {
    if constexpr (std::is_same<Path, vec>::value) {
        constexpr int CD = 24 / P::SPD;
        static_assert(PX == 8, "a vec lane owns 8 pixels");
        uint32_t d[CD];
        load_dwords<CD>(row + (size_t)x * 3u * sizeof(typename P::T), d);
        unpack_codes<P, CD>(d, q);
    } else {
        const typename P::T* __restrict__ s = reinterpret_cast<const typename P::T*>(row) + (size_t)x * 3u;
#pragma unroll
        for (int k = 0; k < 3 * PX; ++k) q[k] = P::code(s[k]);
    }
}

// One block: TILE_ROWS rows x 64 * PX columns of one frame.  A wave walks its WAVE_ROWS rows top to bottom with the luma of rows y - 1, y,
// y + 1 in registers (a one-row halo on either side); what it adds to the record in global memory is bounded by the tile, not by its content:
// one atomic per row per wave, one per column, bin and scalar per block.
template <class P, class Path>
__device__ __forceinline__ void probe_tile(const Args& a) {
    constexpr int PX = std::is_same<Path, vec>::value ? 8 : 1, COLS = 64 * PX;
    __shared__ uint32_t hist[256 * COPIES];
    __shared__ uint32_t cols[COLS];
    __shared__ uint32_t part[WAVES][10];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    for (uint32_t i = tid; i < 256u * COPIES; i += BLOCK) hist[i] = 0u;
    for (uint32_t i = tid; i < (uint32_t)COLS; i += BLOCK) cols[i] = 0u;
    __syncthreads();

    const uint32_t x0 = blockIdx.x * COLS, x = x0 + lane * PX;
    const bool act = x < a.w;                                           // vec: w % 8 == 0, so a lane's 8 pixels are in the row or none is
    const size_t row = (size_t)a.w * 3u * sizeof(typename P::T);
    const uint8_t* __restrict__ s = a.src + (size_t)blockIdx.z * a.src_stride;
    const uint8_t* __restrict__ pv = blockIdx.z ? s - a.src_stride : a.prev;       // P: the frame before C in the batch, or the caller's
    uint32_t* __restrict__ rec = reinterpret_cast<uint32_t*>(a.dst + (size_t)blockIdx.z * a.dst_stride);
    const uint32_t r0 = blockIdx.y * TILE_ROWS + wv * WAVE_ROWS, r1 = r0 + WAVE_ROWS < a.h ? r0 + WAVE_ROWS : a.h;

    uint32_t mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
    uint32_t sum = 0u, s_cur = 0u, s_even = 0u, s_odd = 0u, colacc[PX];
#pragma unroll
    for (int p = 0; p < PX; ++p) colacc[p] = 0u;

    // the luma of a row; a row of the wave's own (not a halo row) also feeds the channel extremes
    auto luma_row = [&](const uint8_t* __restrict__ frame, uint32_t y, bool own, int (&Y)[PX]) {
        int q[3 * PX];
        load_codes<P, Path, PX>(frame + (size_t)y * row, x, q);
        if constexpr (std::is_same<P, u8>::value) {                    // a uint8 sample u has the code 4 u
#pragma unroll
            for (int k = 0; k < 3 * PX; ++k) q[k] *= 4;
        }
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            Y[p] = luma(q[3 * p], q[3 * p + 1], q[3 * p + 2]);
            if (own) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const uint32_t c = (uint32_t)q[3 * p + k];
                    mn[k] = c < mn[k] ? c : mn[k];
                    mx[k] = c > mx[k] ? c : mx[k];
                }
            }
        }
    };

    if (r0 < a.h) {                                                     // wave-uniform: lane 0 of such a wave is always in the row (x0 < w)
        int Yu[PX], Yc[PX], Yd[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) Yu[p] = Yc[p] = Yd[p] = 0;
        if (act) {
            luma_row(s, r0, true, Yc);
            if (r0 > 0u) luma_row(s, r0 - 1u, false, Yu);
        }
        for (uint32_t y = r0; y < r1; ++y) {
            const bool below = y + 1u < a.h, inner = y > 0u && below;
            if (act && below) luma_row(s, y + 1u, y + 1u < r1, Yd);
            uint32_t rs = 0u;
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                const uint32_t Y = (uint32_t)Yc[p], bin = Y >> 2;
                rs += Y;
                colacc[p] += Y;
                // a wave whose lanes all hold one bin (a flat picture) adds their count once; else each lane adds to its own sub-histogram
                const uint32_t b0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)bin);
                const uint32_t lanes = (uint32_t)__popcll(__ballot(act));         // counted here, where the whole wave votes
                if (__all(!act || bin == b0)) {
                    if (lane == 0u) atomicAdd(&hist[b0 * COPIES], lanes);
                } else if (act) {
                    atomicAdd(&hist[bin * COPIES + (lane & (COPIES - 1))], 1u);
                }
            }
            sum += rs;
            if (inner && act) {
#pragma unroll
                for (int p = 0; p < PX; ++p) {
                    const int t = Yu[p] + Yd[p] - 2 * Yc[p];
                    s_cur += (uint32_t)(t < 0 ? -t : t);
                }
                if (pv) {
                    int Yp[PX];
                    luma_row(pv, y, false, Yp);
                    uint32_t acc = 0u;
#pragma unroll
                    for (int p = 0; p < PX; ++p) {
                        const int t = Yu[p] + Yd[p] - 2 * Yp[p];
                        acc += (uint32_t)(t < 0 ? -t : t);
                    }
                    if (y & 1u) s_odd += acc; else s_even += acc;
                }
            }
            rs = wave_sum(rs);                                          // lanes past the row hold 0
            if (lane == 0u && rs) atomicAdd(&rec[W_ROWS + y], rs);
#pragma unroll
            for (int p = 0; p < PX; ++p) { Yu[p] = Yc[p]; Yc[p] = Yd[p]; }
        }
        if (act) {
#pragma unroll
            for (int p = 0; p < PX; ++p) atomicAdd(&cols[lane * PX + p], colacc[p]);
        }
    }
    // per lane: sum <= 8 * 8 * 1020, an S sum <= 8 * 8 * 2040; per block 256 lanes: below 2^26
    {
        const uint32_t v[10] = {wave_min(mn[0]), wave_min(mn[1]), wave_min(mn[2]), wave_max(mx[0]), wave_max(mx[1]), wave_max(mx[2]),
                                wave_sum(sum), wave_sum(s_cur), wave_sum(s_even), wave_sum(s_odd)};
        if (lane == 0u) {
#pragma unroll
            for (int k = 0; k < 10; ++k) part[wv][k] = v[k];
        }
    }
    __syncthreads();
    if (tid < 10u) {
        uint32_t v = part[0][tid];
        for (int k = 1; k < WAVES; ++k) {
            const uint32_t t = part[k][tid];
            v = tid < 3u ? (t < v ? t : v) : tid < 6u ? (t > v ? t : v) : v + t;
        }
        if (tid < 3u) { if (v != 0xffffffffu) atomicMin(&rec[W_MIN + tid], v); }
        else if (tid < 6u) { if (v) atomicMax(&rec[W_MAX + tid - 3u], v); }
        else if (v) atomicAdd(reinterpret_cast<unsigned long long*>(rec + W_SUM + 2u * (tid - 6u)), (unsigned long long)v);
    }
    {
        uint32_t v = 0u;                                                // BLOCK == 256 bins: one per thread
#pragma unroll
        for (int c = 0; c < COPIES; ++c) v += hist[tid * COPIES + ((c + tid) & (COPIES - 1))];
        if (v) atomicAdd(&rec[W_HIST + tid], v);
    }
    for (uint32_t c = tid; c < (uint32_t)COLS; c += BLOCK) {
        const uint32_t v = cols[c];
        if (x0 + c < a.w && v) atomicAdd(&rec[W_ROWS + a.h + x0 + c], v);
    }
}

template <class P, class Path>
__global__ __launch_bounds__(BLOCK) void k_probe(Args a) {
    static_assert(BLOCK == 256, "one histogram bin per thread");
    probe_tile<P, Path>(a);
}

// every word of every record of a launch: the flags, the minima at their identity, zeros
__global__ __launch_bounds__(BLOCK) void k_probe_init(Args a) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.words) return;
    uint32_t* __restrict__ rec = reinterpret_cast<uint32_t*>(a.dst + (size_t)blockIdx.z * a.dst_stride);
    rec[i] = i == W_FLAGS ? ((blockIdx.z || a.prev) ? 1u : 0u) : (i >= W_MIN && i < W_MAX) ? 0xffffffffu : 0u;
}

}  // namespace crtfx_probe_impl

using namespace crtfx_probe_impl;

struct crtfx_probe : crtfx_frames::Plan {      // the record is the output frame: dst_bytes = 4 * words, one per source frame
    int h = 0, w = 0;
    bool half = false;
};

namespace {

using crtfx_frames::Batch;
using crtfx_stage::create_err;
using crtfx_stage::fail;

template <class P>
void launch_path(bool fits, dim3 grid, hipStream_t st, const Args& a) {
    if (fits) hipLaunchKernelGGL((k_probe<P, vec>), grid, dim3(BLOCK), 0, st, a);
    else hipLaunchKernelGGL((k_probe<P, general>), grid, dim3(BLOCK), 0, st, a);
}

struct U : crtfx_frames::Unit {
    using H = crtfx_probe;
    static constexpr int force_option = CRTFX_PROBE_OPT_FORCE_GENERAL;
    static constexpr const char* name = "probe";

    // the vec kernels' conditions (crtfx_probe.h); the records are multiples of 8 on either path
    static bool vec_fits(const H* p, const Batch& b) {
        if (p->force_general || (p->w & 7)) return false;
        if ((reinterpret_cast<uintptr_t>(b.src) | reinterpret_cast<uintptr_t>(b.prev)) & 3u) return false;
        return b.n <= 1 || !(b.src_stride & 3u);
    }

    static void note_plan(H* p, bool fits, int frames) {
        snprintf(p->plan, sizeof p->plan, "probe=k_probe<%s,%s>;frames=%d", p->half ? f16::name : u8::name, fits ? vec::name : general::name, frames);
    }

    static Args make_args(const H* p, bool, const Batch& b) {
        Args a{};
        a.prev = static_cast<const uint8_t*>(b.prev);
        a.h = (uint32_t)p->h; a.w = (uint32_t)p->w;
        a.words = (uint32_t)(p->dst_bytes / 4);
        return a;
    }

    static void launch(const H* p, bool fits, Args& a, int f, unsigned g, hipStream_t st) {
        if (f) a.prev = a.src - a.src_stride;                           // a later group: the last frame of the group before it
        hipLaunchKernelGGL(k_probe_init, dim3((a.words + BLOCK - 1) / BLOCK, 1, g), dim3(BLOCK), 0, st, a);
        const uint32_t cols = fits ? 512u : 64u;
        const dim3 grid((a.w + cols - 1) / cols, (a.h + TILE_ROWS - 1) / TILE_ROWS, g);
        if (p->half) launch_path<f16>(fits, grid, st, a); else launch_path<u8>(fits, grid, st, a);
    }
};

}  // namespace

extern "C" {

const char* crtfx_probe_last_error(const crtfx_probe* p) { return p ? p->err.c_str() : create_err<crtfx_probe>().c_str(); }

size_t crtfx_probe_words(int h, int w) {
    if (h < 1 || h > 32767 || w < 1 || w > 32767) return 0;
    return ((size_t)W_ROWS + (size_t)h + (size_t)w + 1u) & ~(size_t)1u;
}

int crtfx_probe_create(int device, int h, int w, int pix_fmt, crtfx_probe** out_plan) {
    using H = crtfx_probe;
    if (const int rc = crtfx_frames::begin_create(out_plan)) return rc;
    if (const int rc = crtfx_frames::check_size<H>("h", h)) return rc;
    if (const int rc = crtfx_frames::check_size<H>("w", w)) return rc;
    if (pix_fmt != CRTFX_PIX_U8 && pix_fmt != CRTFX_PIX_F16) return fail<H>(nullptr, CRTFX_E_INVALID, "unknown pix_fmt %d", pix_fmt);
    return crtfx_frames::new_plan<U>(device, out_plan, [&](H* p) {
        p->h = h; p->w = w;
        p->half = pix_fmt == CRTFX_PIX_F16;
        p->src_bps = p->half ? 2 : 1;
        p->dst_bps = 1;                                                 // the records' own alignment rule is crtfx_probe_run's
        p->src_bytes = (size_t)h * w * 3 * p->src_bps;
        p->dst_bytes = 4 * crtfx_probe_words(h, w);
        return CRTFX_OK;
    });
}

int crtfx_probe_destroy(crtfx_probe* p) { return crtfx_frames::destroy(p); }

int crtfx_probe_set_option(crtfx_probe* p, int option, int value) { return crtfx_frames::set_option<U>(p, option, value); }

int crtfx_probe_last_plan(crtfx_probe* p, char* buf, size_t n) { return crtfx_frames::last_plan(p, buf, n); }

int crtfx_probe_run(crtfx_probe* p, const void* prev_frame, const void* src_base, size_t src_stride_bytes, void* records, size_t record_stride_bytes,
                    int n, void* stream) {
    if (!p) return CRTFX_E_INVALID;
    if (n > 0 && records && ((reinterpret_cast<uintptr_t>(records) & 7u) || (n > 1 && (record_stride_bytes & 7u))))
        return fail(p, CRTFX_E_INVALID, "records need a base and a stride that are multiples of 8 (the 64-bit sums)");
    return crtfx_frames::run<U>(p, Batch{prev_frame, src_base, src_stride_bytes, records, record_stride_bytes, n}, stream);
}

}  // extern "C"
