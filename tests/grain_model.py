"""Host model of the in-kernel film-grain generator (stage a11, ref:635-647), restated in float64 numpy.

cv2.randn cannot be reproduced, so the library draws its own N(0, 1) plane from a counter-based hash (crtfx_common.hip.h
grain_normal, keyed by crtfx.hip noise_keys).  This module states that generator from its description, with none of the
library's code or float32 arithmetic, so that the GPU's planes have something outside the GPU to be compared with:

  * mix32 (= lowbias32): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16, on uint32 with wrap-around;
  * noise_keys(seed, frame): (k0, k1) from the 32-bit halves s0, s1 of the seed and f0, f1 of the frame index;
  * uniforms(k0, k1, idx): a = mix32(idx ^ k0) ^ k1, u1 = ((a >> 16) + 1) / 2^16 in (0, 1], u2 = (a & 0xFFFF) / 2^16 in [0, 1);
  * plane(seed, frame, h, w): z = sqrt(-2 ln u1) cos(2 pi u2) at idx = y * w + x (also the coarse grain grid (h // g, w // g)).

Only numpy: nothing here imports the package or the oracle."""
import numpy as np

M32 = 0xFFFFFFFF
C1, C2 = 0x7FEB352D, 0x846CA68B                       # lowbias32's multipliers
C1_INV, C2_INV = 0x1D69E2A5, 0x43021123               # their inverses mod 2^32 (the standard lowbias32 inverse)
GOLDEN, F1_ADD, S1_ADD = 0x9E3779B9, 0x85EBCA6B, 0xC2B2AE35
INV_2_16 = 2.0 ** -16
CHUNK = 1 << 20                                       # pixels per step of plane(): bounded memory at 4K and above


def mix32(x):
    """lowbias32 on uint32 words (any shape; a Python int gives a 0-d array).  The products are formed in uint64, where
    two 32-bit factors cannot overflow, and reduced mod 2^32."""
    x = np.asarray(x).astype(np.uint64) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(C1)) & np.uint64(M32)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(C2)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def mix32_inverse(x):
    """The inverse of mix32: undo each step in reverse order (x ^= x >> 15 is undone by x ^= (x >> 15) ^ (x >> 30))."""
    x = np.asarray(x).astype(np.uint64) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(C2_INV)) & np.uint64(M32)
    x ^= (x >> np.uint64(15)) ^ (x >> np.uint64(30))
    x = (x * np.uint64(C1_INV)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def _mix(v: int) -> int:
    return int(mix32(v & M32))


def noise_keys(seed: int, frame: int):
    """(k0, k1) for a seed and a frame index, each any integer in [0, 2^64); both halves of both enter the keys."""
    seed, frame = int(seed), int(frame)
    if not (0 <= seed < 1 << 64 and 0 <= frame < 1 << 64):
        raise ValueError("seed and frame must lie in [0, 2^64)")
    s0, s1 = seed & M32, seed >> 32
    f0, f1 = frame & M32, frame >> 32
    k0 = _mix(s0 ^ _mix(f0 + GOLDEN) ^ _mix(f1 + F1_ADD))
    k1 = _mix(s1 + S1_ADD + _mix(k0 ^ f0))
    return k0, k1


def uniforms(k0: int, k1: int, idx):
    """-> (u1, u2) as float64 arrays: u1 in (0, 1], u2 in [0, 1), both multiples of 2^-16 (exact in float32 too)."""
    a = mix32(np.asarray(idx).astype(np.uint32) ^ np.uint32(k0)) ^ np.uint32(k1)
    u1 = ((a >> np.uint32(16)).astype(np.float64) + 1.0) * INV_2_16
    u2 = (a & np.uint32(0xFFFF)).astype(np.float64) * INV_2_16
    return u1, u2


def box_muller(u1, u2):
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def plane(seed: int, frame: int, h: int, w: int, with_u1: bool = False):
    """The (h, w) float64 N(0, 1) plane of frame `frame` under `seed` (pixel index y * w + x).  with_u1: also return u1."""
    n = int(h) * int(w)
    assert 0 < n <= 1 << 32
    k0, k1 = noise_keys(seed, frame)
    z = np.empty(n, dtype=np.float64)
    u1_all = np.empty(n, dtype=np.float64) if with_u1 else None
    for lo in range(0, n, CHUNK):
        hi = min(n, lo + CHUNK)
        u1, u2 = uniforms(k0, k1, np.arange(lo, hi, dtype=np.uint64).astype(np.uint32))
        z[lo:hi] = box_muller(u1, u2)
        if with_u1:
            u1_all[lo:hi] = u1
    z = z.reshape(h, w)
    return (z, u1_all.reshape(h, w)) if with_u1 else z


def planes(seed: int, first: int, n: int, h: int, w: int, grain_size: int = 1):
    """The float32 planes the oracle takes for frames first .. first + n - 1 (the coarse grid when grain_size > 1)."""
    if grain_size > 1:
        h, w = max(1, h // grain_size), max(1, w // grain_size)
    return [plane(seed, (first + j) & ((1 << 64) - 1), h, w).astype(np.float32) for j in range(n)]
