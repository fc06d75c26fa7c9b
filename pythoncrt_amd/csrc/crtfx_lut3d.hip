// crtfx_lut3d.hip — the 3D LUT stage (include/crtfx_lut3d.h): uint8 or half RGB frames through a colour cube with tetrahedral
// interpolation.  One kernel body in eight builds — sample type x where the cube lives (LDS / device memory) x how a lane walks pixels
// (4 per lane / 1 per lane) — the host glue, the C entry points.

#include <hip/hip_runtime.h>

#include <cstdio>
#include <type_traits>
#include <vector>

#include "crtfx_lut3d.h"
#include "crtfx_frame_host.h"

namespace crtfx_lut3d_impl {

struct u8 { static constexpr const char* name = "u8"; static constexpr uint32_t S = 255u, bytes = 1u; };
struct half { static constexpr const char* name = "half"; static constexpr uint32_t S = 1020u, bytes = 2u; };
struct lds { static constexpr const char* name = "lds"; };
struct global { static constexpr const char* name = "global"; };
struct vec { static constexpr const char* name = "vec"; };
struct general { static constexpr const char* name = "general"; };

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef u32x4 u32x4_dword_aligned __attribute__((aligned(4)));          // a 16-byte access at a dword-aligned address
typedef u32x2 u32x2_dword_aligned __attribute__((aligned(4)));          // an 8-byte one

// Launch constants.
struct Args {
    const uint8_t* src;
    uint8_t* dst;
    size_t src_stride, dst_stride;      // bytes
    const uint32_t* table;              // the packed cube in device memory: r | g << 10 | b << 20, red fastest; padded to whole 16 bytes
    uint32_t cube;                      // N^3 entries
    uint32_t N;
    uint32_t pixels;                    // of one frame (below 2^30)
    uint32_t items;                     // lanes' work items of one frame: vec ceil(pixels / 4), general pixels
    uint32_t frames;                    // of this launch: frames * items < 2^31
};

constexpr int BLOCK = 1024;
constexpr uint32_t QMAX = CRTFX_LUT3D_QMAX;

extern __shared__ __attribute__((aligned(16))) uint32_t cube_lds[];     // lds builds: the packed cube, 4 * N^3 bytes of dynamic LDS

// q = rint_to_even(min(max(4 f, 0), 1020)), NaN -> 0: crtfx_resize16.h's `in:` quantiser (crtfx_resize16.hip), word for word
__device__ __forceinline__ uint32_t quantise(uint32_t bits16) {
    float t = 4.0f * (float)__builtin_bit_cast(_Float16, (unsigned short)bits16);
    t = t > 0.0f ? t : 0.0f;
    t = t < 1020.0f ? t : 1020.0f;
    return (uint32_t)(int)rintf(t);
}

// the half bit pattern of quarter code q, q / 4 on the 0..255 scale: exact, every quarter code is a half
__device__ __forceinline__ uint32_t half_bits(uint32_t q) { return (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)((float)q * 0.25f)); }

template <class T> __device__ __forceinline__ uint32_t sample_in(uint32_t raw) {
    if constexpr (std::is_same<T, half>::value) return quantise(raw); else return raw;
}
template <class T> __device__ __forceinline__ uint32_t sample_out(uint32_t code) {
    if constexpr (std::is_same<T, half>::value) return half_bits(code); else return code;
}

template <class M> __device__ __forceinline__ uint32_t entry(const uint32_t* __restrict__ table, uint32_t idx) {
    if constexpr (std::is_same<M, lds>::value) return cube_lds[idx]; else return table[idx];
}

// order (fa, ea), (fb, eb) so that fa >= fb
__device__ __forceinline__ void order(uint32_t& fa, uint32_t& ea, uint32_t& fb, uint32_t& eb) {
    const bool sw = fa < fb;
    const uint32_t f = sw ? fb : fa, e = sw ? eb : ea;
    fb = sw ? fa : fb; eb = sw ? ea : eb;
    fa = f; ea = e;
}

// One pixel: x0, x1, x2 = r, g, b in 0..S -> the three output codes.  Every index is below N^3 whatever x holds: i <= N - 2 per axis.
template <class T, class M>
__device__ __forceinline__ void lut_pixel(const Args& a, uint32_t NN, uint32_t x0, uint32_t x1, uint32_t x2, uint32_t& o0, uint32_t& o1, uint32_t& o2) {
    constexpr uint32_t S = T::S;
    const uint32_t n1 = a.N - 1u, n2 = a.N - 2u;
    const uint32_t m0 = x0 * n1, m1 = x1 * n1, m2 = x2 * n1;            // <= 1020 * 64
    const uint32_t i0 = min(m0 / S, n2), i1 = min(m1 / S, n2), i2 = min(m2 / S, n2);
    uint32_t f0 = m0 - i0 * S, f1 = m1 - i1 * S, f2 = m2 - i2 * S;      // 0..S
    uint32_t e0 = 1u, e1 = a.N, e2 = NN;
    const uint32_t idx = i0 + a.N * i1 + NN * i2;
    order(f0, e0, f1, e1);
    order(f1, e1, f2, e2);
    order(f0, e0, f1, e1);                                              // f0 >= f1 >= f2
    const uint32_t t0 = entry<M>(a.table, idx), t1 = entry<M>(a.table, idx + e0), t2 = entry<M>(a.table, idx + e0 + e1),
                   t3 = entry<M>(a.table, idx + 1u + a.N + NN);
    const uint32_t w0 = S - f0, w1 = f0 - f1, w2 = f1 - f2, w3 = f2;    // sum S
    uint32_t o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t sh = 10u * c;
        const uint32_t sum = __umul24(w0, (t0 >> sh) & 1023u) + __umul24(w1, (t1 >> sh) & 1023u) + __umul24(w2, (t2 >> sh) & 1023u)
                           + __umul24(w3, (t3 >> sh) & 1023u);         // <= 1020 * 1020
        o[c] = (sum + 510u) / 1020u;
    }
    o0 = o[0]; o1 = o[1]; o2 = o[2];
}

// general, and the tail of a vec frame: pixel p of the frame at s / d, element by element
template <class T, class M>
__device__ __forceinline__ void one_pixel(const Args& a, uint32_t NN, const uint8_t* __restrict__ s, uint8_t* __restrict__ d, uint32_t p) {
    uint32_t r[3];
    if constexpr (std::is_same<T, half>::value) {
        const uint16_t* ss = reinterpret_cast<const uint16_t*>(s) + (size_t)p * 3u;
        r[0] = ss[0]; r[1] = ss[1]; r[2] = ss[2];
    } else {
        const uint8_t* ss = s + (size_t)p * 3u;
        r[0] = ss[0]; r[1] = ss[1]; r[2] = ss[2];
    }
    uint32_t o0, o1, o2;
    lut_pixel<T, M>(a, NN, sample_in<T>(r[0]), sample_in<T>(r[1]), sample_in<T>(r[2]), o0, o1, o2);
    if constexpr (std::is_same<T, half>::value) {
        uint16_t* dd = reinterpret_cast<uint16_t*>(d) + (size_t)p * 3u;
        dd[0] = (uint16_t)half_bits(o0); dd[1] = (uint16_t)half_bits(o1); dd[2] = (uint16_t)half_bits(o2);
    } else {
        uint8_t* dd = d + (size_t)p * 3u;
        dd[0] = (uint8_t)o0; dd[1] = (uint8_t)o1; dd[2] = (uint8_t)o2;
    }
}

// vec: item j of a frame is its pixels 4 j .. 4 j + 3 (12 samples: 3 dwords of uint8, 6 of halves); the frame's last, short item goes by pixel
template <class T, class M>
__device__ __forceinline__ void four_pixels(const Args& a, uint32_t NN, const uint8_t* __restrict__ s, uint8_t* __restrict__ d, uint32_t j) {
    const uint32_t p0 = j * 4u;
    if (p0 + 4u > a.pixels) {
#pragma unroll 1
        for (uint32_t p = p0; p < a.pixels; ++p) one_pixel<T, M>(a, NN, s, d, p);
        return;
    }
    constexpr uint32_t W = 3u * T::bytes;                              // dwords of the item
    constexpr uint32_t PER = 4u / T::bytes, BITS = 8u * T::bytes, MASK = (1u << BITS) - 1u;
    uint32_t in[W], out[W];
    const uint8_t* ss = s + (size_t)j * (4u * W);
    uint8_t* dd = d + (size_t)j * (4u * W);
    if constexpr (std::is_same<T, half>::value) {
        const u32x4 lo = *reinterpret_cast<const u32x4_dword_aligned*>(ss);
        const u32x2 hi = *reinterpret_cast<const u32x2_dword_aligned*>(ss + 16);
        in[0] = lo.x; in[1] = lo.y; in[2] = lo.z; in[3] = lo.w; in[4] = hi.x; in[5] = hi.y;
    } else {
        const uint32_t* sw = reinterpret_cast<const uint32_t*>(ss);
        in[0] = sw[0]; in[1] = sw[1]; in[2] = sw[2];
    }
#pragma unroll
    for (uint32_t k = 0; k < W; ++k) out[k] = 0u;
#pragma unroll
    for (uint32_t p = 0; p < 4u; ++p) {
        uint32_t x[3], o[3];
#pragma unroll
        for (uint32_t c = 0; c < 3u; ++c) {
            const uint32_t k = 3u * p + c;                              // sample k of the item
            x[c] = sample_in<T>((in[k / PER] >> (BITS * (k % PER))) & MASK);
        }
        lut_pixel<T, M>(a, NN, x[0], x[1], x[2], o[0], o[1], o[2]);
#pragma unroll
        for (uint32_t c = 0; c < 3u; ++c) {
            const uint32_t k = 3u * p + c;
            out[k / PER] |= sample_out<T>(o[c]) << (BITS * (k % PER));
        }
    }
    if constexpr (std::is_same<T, half>::value) {
        const u32x4 lo = {out[0], out[1], out[2], out[3]};
        const u32x2 hi = {out[4], out[5]};
        *reinterpret_cast<u32x4_dword_aligned*>(dd) = lo;
        *reinterpret_cast<u32x2_dword_aligned*>(dd + 16) = hi;
    } else {
        uint32_t* dw = reinterpret_cast<uint32_t*>(dd);
        dw[0] = out[0]; dw[1] = out[1]; dw[2] = out[2];
    }
}

template <class T, class M, class P>
__global__ __launch_bounds__(BLOCK) void k_lut3d(Args a) {
    if constexpr (std::is_same<M, lds>::value) {                        // every lane of the block takes part, whatever its share of the pixels
        const uint32_t quads = (a.cube + 3u) >> 2;                      // the device table and the LDS block are padded to whole 16 bytes
        for (uint32_t k = threadIdx.x; k < quads; k += BLOCK)
            reinterpret_cast<u32x4*>(cube_lds)[k] = reinterpret_cast<const u32x4*>(a.table)[k];
        __syncthreads();
    }
    const uint32_t NN = a.N * a.N;
    const uint32_t total = a.frames * a.items, stride = gridDim.x * BLOCK;      // total < 2^31, stride <= 2^20: no wrap below
    uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= total) return;
    uint32_t f = i / a.items, j = i - f * a.items;
    const uint32_t sf = stride / a.items, sj = stride - sf * a.items;
    for (; i < total; i += stride) {
        const uint8_t* __restrict__ s = a.src + (size_t)f * a.src_stride;
        uint8_t* __restrict__ d = a.dst + (size_t)f * a.dst_stride;
        if constexpr (std::is_same<P, vec>::value) four_pixels<T, M>(a, NN, s, d, j); else one_pixel<T, M>(a, NN, s, d, j);
        j += sj; f += sf;
        if (j >= a.items) { j -= a.items; ++f; }
    }
}

}  // namespace crtfx_lut3d_impl

using namespace crtfx_lut3d_impl;

struct crtfx_lut3d : crtfx_frames::Plan {      // one frame size and sample type on both sides
    int h = 0, w = 0, N = 0;
    bool half = false;
    uint32_t cube = 0;                  // N^3
    size_t lds_bytes = 0;               // 4 * N^3 rounded up to 16; 0 where the cube does not fit a CU's LDS
    size_t pixels = 0;
    uint32_t* table = nullptr;          // device: the packed cube
    int cus = 0;
    bool force_global = false;
    ~crtfx_lut3d() { if (table) (void)hipFree(table); }
};

namespace {

using crtfx_frames::Batch;
using crtfx_stage::DeviceGuard;
using crtfx_stage::create_err;
using crtfx_stage::fail;

using H = crtfx_lut3d;

// The default table path of an N (crtfx_lut3d.h, the timing block): lds wherever the cube fits a CU's LDS.
bool lds_default(int N) { return N <= CRTFX_LUT3D_LDS_MAX_N; }

bool use_lds(const H* p) { return !p->force_global && lds_default(p->N); }

// -1, or the index of the first entry above 1020
long long bad_entry(int N, const uint16_t* table) {
    const long long count = (long long)N * N * N * 3;
    for (long long k = 0; k < count; ++k)
        if (table[k] > CRTFX_LUT3D_QMAX) return k;
    return -1;
}

template <class Hh>
int check_table(Hh* p, int N, const uint16_t* table) {
    if (!table) return fail<H>(p, CRTFX_E_INVALID, "table is null");
    const long long bad = bad_entry(N, table);
    if (bad >= 0) return fail<H>(p, CRTFX_E_INVALID, "table entry %lld = %u above %d", bad, (unsigned)table[bad], CRTFX_LUT3D_QMAX);
    return CRTFX_OK;
}

// r | g << 10 | b << 20 per entry, padded with zeros to whole 16 bytes
std::vector<uint32_t> pack(int N, const uint16_t* table) {
    const size_t cube = (size_t)N * N * N;
    std::vector<uint32_t> v((cube + 3) & ~(size_t)3, 0u);
    for (size_t k = 0; k < cube; ++k) v[k] = (uint32_t)table[3 * k] | (uint32_t)table[3 * k + 1] << 10 | (uint32_t)table[3 * k + 2] << 20;
    return v;
}

template <class T, class M>
void launch_walk(bool vec_path, dim3 grid, size_t shmem, hipStream_t st, const Args& a) {
    if (vec_path) hipLaunchKernelGGL((k_lut3d<T, M, vec>), grid, dim3(BLOCK), shmem, st, a);
    else hipLaunchKernelGGL((k_lut3d<T, M, general>), grid, dim3(BLOCK), shmem, st, a);
}

template <class T>
void launch_table(bool in_lds, bool vec_path, dim3 grid, size_t shmem, hipStream_t st, const Args& a) {
    if (in_lds) launch_walk<T, lds>(vec_path, grid, shmem, st, a);
    else launch_walk<T, global>(vec_path, grid, 0, st, a);
}

// Above 64 KiB a kernel's dynamic LDS limit has to be raised before it is launched.  The limit belongs to the kernel function on the
// device, not to a plan: it is always raised to the whole CU's LDS and never lowered, so plans of different N live side by side.
template <class T>
hipError_t raise_lds_limit() {
    const int bytes = CRTFX_LUT3D_LDS_BYTES;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_lut3d<T, lds, vec>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_lut3d<T, lds, general>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

// the table of a new plan, with the plan's device current
hipError_t upload(H* p, const std::vector<uint32_t>& packed) {
    hipError_t e = hipDeviceGetAttribute(&p->cus, hipDeviceAttributeMultiprocessorCount, p->device);
    if (e == hipSuccess && p->cus < 1) p->cus = 1;
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&p->table), packed.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(p->table, packed.data(), packed.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && p->lds_bytes > 65536) e = p->half ? raise_lds_limit<half>() : raise_lds_limit<u8>();
    return e;
}

struct U : crtfx_frames::Unit {
    using H = crtfx_lut3d;
    static constexpr const char* name = "lut3d";
    static constexpr bool one_size = true;

    // the vec walk's conditions (crtfx_lut3d.h)
    static bool vec_fits(const H* p, const Batch& b) {
        if (p->force_general) return false;
        if ((reinterpret_cast<uintptr_t>(b.src) | reinterpret_cast<uintptr_t>(b.dst)) & 3u) return false;
        return b.n <= 1 || !((b.src_stride | b.dst_stride) & 3u);
    }

    static void note_plan(H* p, bool vec_path, int frames) {
        const bool l = use_lds(p);
        snprintf(p->plan, sizeof p->plan, "lut3d=k_lut3d<%s,%s,%s>;n=%d;lds=%zu;frames=%d", p->half ? half::name : u8::name, l ? lds::name : global::name,
                 vec_path ? vec::name : general::name, p->N, l ? (size_t)p->cube * 4u : (size_t)0, frames);
    }

    static Args make_args(const H* p, bool fits, const Batch&) {
        Args a{};
        a.table = p->table; a.cube = p->cube; a.N = (uint32_t)p->N;
        a.pixels = (uint32_t)p->pixels;                                 // 32767^2 < 2^30
        a.items = fits ? (a.pixels + 3u) / 4u : a.pixels;
        return a;
    }

    static int group(const Args& a) { return (int)(0x7fffffffu / a.items); }       // frames of one launch: frames * items < 2^31

    static void launch(const H* p, bool fits, Args& a, int, unsigned g, hipStream_t st) {
        const bool in_lds = use_lds(p);
        const unsigned per_cu = in_lds ? (CRTFX_LUT3D_LDS_BYTES / p->lds_bytes < 2 ? 1u : 2u) : 2u;        // blocks of 1024 lanes: two fill a CU
        a.frames = g;
        const unsigned need = (a.frames * a.items + BLOCK - 1) / BLOCK, most = (unsigned)p->cus * per_cu;
        const dim3 grid(need < most ? need : most);
        if (p->half) launch_table<half>(in_lds, fits, grid, p->lds_bytes, st, a); else launch_table<u8>(in_lds, fits, grid, p->lds_bytes, st, a);
    }
};

}  // namespace

extern "C" {

const char* crtfx_lut3d_last_error(const crtfx_lut3d* p) { return p ? p->err.c_str() : create_err<H>().c_str(); }

int crtfx_lut3d_create(int device, int h, int w, int pix_fmt, int N, const uint16_t* table, crtfx_lut3d** out_plan) {
    if (const int rc = crtfx_frames::begin_create(out_plan)) return rc;
    if (pix_fmt != CRTFX_PIX_U8 && pix_fmt != CRTFX_PIX_F16) return fail<H>(nullptr, CRTFX_E_INVALID, "unknown pix_fmt %d", pix_fmt);
    if (const int rc = crtfx_frames::check_size<H>("h", h)) return rc;
    if (const int rc = crtfx_frames::check_size<H>("w", w)) return rc;
    if (N < CRTFX_LUT3D_MIN_N || N > CRTFX_LUT3D_MAX_N) return fail<H>(nullptr, CRTFX_E_INVALID, "N = %d outside %d..%d", N, CRTFX_LUT3D_MIN_N, CRTFX_LUT3D_MAX_N);
    if (const int rc = check_table<H>(nullptr, N, table)) return rc;
    return crtfx_frames::new_plan<U>(device, out_plan, [&](H* p) -> int {
        p->h = h; p->w = w; p->N = N; p->half = pix_fmt == CRTFX_PIX_F16;
        p->cube = (uint32_t)N * N * N;
        p->pixels = (size_t)h * w;
        p->src_bps = p->dst_bps = p->half ? 2 : 1;
        p->src_bytes = p->dst_bytes = p->pixels * 3 * p->src_bps;
        const std::vector<uint32_t> packed = pack(N, table);
        p->lds_bytes = lds_default(N) ? packed.size() * 4 : 0;
        const hipError_t e = upload(p, packed);
        if (e != hipSuccess) return fail<H>(nullptr, e == hipErrorOutOfMemory ? CRTFX_E_NOMEM : CRTFX_E_HIP, "lut3d create: %s", hipGetErrorString(e));
        return CRTFX_OK;
    });
}

int crtfx_lut3d_destroy(crtfx_lut3d* p) { return crtfx_frames::destroy(p); }

int crtfx_lut3d_set_table(crtfx_lut3d* p, int N, const uint16_t* table) {
    if (!p) return CRTFX_E_INVALID;
    if (N != p->N) return fail(p, CRTFX_E_INVALID, "N = %d differs from the plan's N = %d", N, p->N);
    if (const int rc = check_table(p, N, table)) return rc;
    const std::vector<uint32_t> packed = pack(N, table);
    DeviceGuard guard(p->device);
    if (guard.err != hipSuccess) return fail(p, CRTFX_E_HIP, "hipSetDevice(%d): %s", p->device, hipGetErrorString(guard.err));
    hipError_t e = hipDeviceSynchronize();                              // the runs already enqueued read the old cube
    if (e == hipSuccess) e = hipMemcpy(p->table, packed.data(), packed.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(p, CRTFX_E_HIP, "lut3d set_table: %s", hipGetErrorString(e));
    return CRTFX_OK;
}

// two options: an entry point of its own
int crtfx_lut3d_set_option(crtfx_lut3d* p, int option, int value) {
    if (!p) return CRTFX_E_INVALID;
    if (option != CRTFX_LUT3D_OPT_FORCE_GENERAL && option != CRTFX_LUT3D_OPT_FORCE_GLOBAL) return fail(p, CRTFX_E_INVALID, "unknown lut3d option %d", option);
    const char* name = option == CRTFX_LUT3D_OPT_FORCE_GENERAL ? "FORCE_GENERAL" : "FORCE_GLOBAL";
    if (value != 0 && value != 1) return fail(p, CRTFX_E_INVALID, "%s takes 0 or 1, got %d", name, value);
    if (option == CRTFX_LUT3D_OPT_FORCE_GENERAL) p->force_general = value != 0; else p->force_global = value != 0;
    U::note_plan(p, U::vec_fits(p, Batch{nullptr, nullptr, 0, nullptr, 0, 1}), 0);
    return CRTFX_OK;
}

int crtfx_lut3d_last_plan(crtfx_lut3d* p, char* buf, size_t n) { return crtfx_frames::last_plan(p, buf, n); }

int crtfx_lut3d_run(crtfx_lut3d* p, const void* src_base, size_t src_stride_bytes, void* dst_base, size_t dst_stride_bytes, int n, void* stream) {
    return crtfx_frames::run<U>(p, Batch{nullptr, src_base, src_stride_bytes, dst_base, dst_stride_bytes, n}, stream);
}

}  // extern "C"

