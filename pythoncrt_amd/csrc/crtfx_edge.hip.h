// crtfx_edge.hip.h — what the deinterlace stages share (include/crtfx_deint.h, include/crtfx_adeint.h): the tags of the field modes and the
// paths, the sample types with the quarter-code quantiser, the dword-multiple loads and stores of the vec paths, and EDGE's direction search.
// crtfx_deint.hip and crtfx_adeint.hip include it, and crtfx_interlace.hip for the sample types and the loads and stores; everything is inlined
// device code in crtfx_deint_impl, and no kernel is declared here.
#ifndef CRTFX_EDGE_HIP_H
#define CRTFX_EDGE_HIP_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace crtfx_deint_impl {

struct first { static constexpr const char* name = "first"; };
struct both { static constexpr const char* name = "both"; };
struct vec { static constexpr const char* name = "vec"; };
struct general { static constexpr const char* name = "general"; };

// q = rint_to_even(min(max(4 f, 0), 1020)), NaN -> 0: crtfx_resize16's quantiser (crtfx_resize16.hip), word for word
__device__ __forceinline__ int quantise(uint32_t bits16) {
    float t = 4.0f * (float)__builtin_bit_cast(_Float16, (unsigned short)bits16);
    t = t > 0.0f ? t : 0.0f;
    t = t < 1020.0f ? t : 1020.0f;
    return (int)rintf(t);
}

// the sample types: the code a sample's bits stand for in the arithmetic, and the bits of a result
struct u8 {
    static constexpr const char* name = "u8";
    typedef uint8_t T;
    static __device__ __forceinline__ int code(uint32_t bits) { return (int)bits; }
    static __device__ __forceinline__ uint32_t bits(int q) { return (uint32_t)q; }
    static constexpr int SPD = 4;       // samples per dword
    static __device__ __forceinline__ void codes(uint32_t dword, int (&q)[SPD]) {      // the codes of a dword's samples, lowest address first
#pragma unroll
        for (int i = 0; i < SPD; ++i) q[i] = (int)((dword >> (8 * i)) & 0xffu);
    }
};
struct f16 {
    static constexpr const char* name = "f16";
    typedef uint16_t T;
    static __device__ __forceinline__ int code(uint32_t bits) { return quantise(bits); }
    // q / 4 on the 0..255 scale: exact, every quarter code is a half
    static __device__ __forceinline__ uint32_t bits(int q) { return (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)((float)q * 0.25f)); }
    static constexpr int SPD = 2;
    // Both samples of a dword at once, in packed half arithmetic, with the codes of code(): 4 f is exact in half unless it overflows, and then
    // it is inf and clipped to 1020 as 4 f is; the maximum with 0 drops a NaN as the comparison does (the product is a quiet one); every
    // integer up to 1020 is a half, so rounding to even in half gives the integer it gives in float.
    static __device__ __forceinline__ void codes(uint32_t dword, int (&q)[SPD]) {
        typedef _Float16 half2 __attribute__((ext_vector_type(2)));
        half2 t = __builtin_bit_cast(half2, dword) * (half2)(_Float16)4.0f;
        t = __builtin_elementwise_max(t, (half2)(_Float16)0.0f);
        t = __builtin_elementwise_min(t, (half2)(_Float16)1020.0f);
        t = __builtin_elementwise_rint(t);
        q[0] = (int)t.x; q[1] = (int)t.y;
    }
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef u32x4 u32x4_dword_aligned __attribute__((aligned(4)));          // a 16-byte access at a dword-aligned address
typedef u32x2 u32x2_dword_aligned __attribute__((aligned(4)));          // an 8-byte one

constexpr int BLOCK = 256;
constexpr int REACH = 3;                // columns the direction search reaches on either side of a pixel

// The direction search of crtfx_deint.h for NP neighbouring pixels.  A and B are the kept rows above and below as codes, pixel i of the NP at
// window index i + REACH; d[i] is the direction taken.  Branch-free: S(2j) counts only behind a successful S(j).
template <int NP>
__device__ __forceinline__ void edge_search(const int (&A)[NP + 2 * REACH][3], const int (&B)[NP + 2 * REACH][3], int (&d)[NP]) {
    int s[NP];
    bool step[NP] = {};
#pragma unroll
    for (int jj = 0; jj < 5; ++jj) {
        constexpr int order[5] = {0, -1, -2, 1, 2};
        const int j = order[jj];
        int D[NP + 2];                  // D[c]: the three channels' |a - b| of the pixel pair centred at window index c + REACH - 1
#pragma unroll
        for (int c = 0; c < NP + 2; ++c) {
            int v = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int t = A[c + REACH - 1 + j][k] - B[c + REACH - 1 - j][k];
                v += t < 0 ? -t : t;
            }
            D[c] = v;
        }
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int S = D[i] + D[i + 1] + D[i + 2];
            if (j == 0) { s[i] = S - 1; d[i] = 0; continue; }
            const bool take = ((j == -1 || j == 1) || step[i]) && S < s[i];
            s[i] = take ? S : s[i];
            d[i] = take ? j : d[i];
            if (j == -1 || j == 1) step[i] = take;
        }
    }
}

// n dwords at a dword-aligned address, as 16-, 8- and 4-byte pieces
template <int N>
__device__ __forceinline__ void load_dwords(const uint8_t* __restrict__ p, uint32_t* out) {
    static_assert(N % 2 == 0 || N == 3, "pieces");
    if constexpr (N == 3) {
        const u32x2 q = *reinterpret_cast<const u32x2_dword_aligned*>(p);
        out[0] = q.x; out[1] = q.y; out[2] = *reinterpret_cast<const uint32_t*>(p + 8);
    } else {
#pragma unroll
        for (int i = 0; i + 4 <= N; i += 4) {
            const u32x4 q = *reinterpret_cast<const u32x4_dword_aligned*>(p + 4 * i);
            out[i] = q.x; out[i + 1] = q.y; out[i + 2] = q.z; out[i + 3] = q.w;
        }
        if constexpr (N % 4 == 2) {
            const u32x2 q = *reinterpret_cast<const u32x2_dword_aligned*>(p + 4 * (N - 2));
            out[N - 2] = q.x; out[N - 1] = q.y;
        }
    }
}

// the codes of N loaded dwords, sample i of them at q[i]
template <class P, int N>
__device__ __forceinline__ void unpack_codes(const uint32_t* w, int* q) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        int t[P::SPD];
        P::codes(w[i], t);
#pragma unroll
        for (int j = 0; j < P::SPD; ++j) q[i * P::SPD + j] = t[j];
    }
}

template <int N>
__device__ __forceinline__ void store_dwords(uint8_t* __restrict__ p, const uint32_t* in) {
    static_assert(N % 2 == 0, "pieces");
#pragma unroll
    for (int i = 0; i + 4 <= N; i += 4) {
        const u32x4 q = {in[i], in[i + 1], in[i + 2], in[i + 3]};
        *reinterpret_cast<u32x4_dword_aligned*>(p + 4 * i) = q;
    }
    if constexpr (N % 4 == 2) {
        const u32x2 q = {in[N - 2], in[N - 1]};
        *reinterpret_cast<u32x2_dword_aligned*>(p + 4 * (N - 2)) = q;
    }
}

}  // namespace crtfx_deint_impl

#endif  // CRTFX_EDGE_HIP_H
