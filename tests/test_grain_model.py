"""CPU: the host model of the grain generator (tests/grain_model.py) — the ranges of its uniforms, the bijection behind its
law, and the separation of its keys over both 32-bit halves of the seed and of the frame index.  tests/test_grain_gpu.py holds
every kernel build's draw to this model."""
import math

import numpy as np
import pytest

from tests import grain_model as gm

N16 = 1 << 16
KEYS = [gm.noise_keys(0, 0), gm.noise_keys(99, 1), gm.noise_keys((1 << 64) - 1, (1 << 33) + 5), gm.noise_keys(0x9E3779B97F4A7C15, 1 << 32)]


def grid_moments():
    """Mean, variance and fourth moment of z over the full 65536 x 65536 grid of (u1, u2): z = r cos(t) with r and t independent,
    so each moment is a product of one sum over the 65536 radii and one over the 65536 angles."""
    u1 = np.arange(1, N16 + 1, dtype=np.float64) / N16
    u2 = np.arange(N16, dtype=np.float64) / N16
    r2 = -2.0 * np.log(u1)
    c = np.cos(2.0 * np.pi * u2)
    m1 = np.sqrt(r2).mean() * c.mean()
    m2 = r2.mean() * (c * c).mean()
    m4 = (r2 * r2).mean() * (c ** 4).mean()
    return m1, m2 - m1 * m1, m4


def idx_for_word(k0, k1, a):
    """The pixel index whose hash word is `a` under keys (k0, k1): mix32 is invertible."""
    return gm.mix32_inverse(np.uint32(a) ^ np.uint32(k1)) ^ np.uint32(k0)


def test_mix32_constants_and_inverse():
    assert (gm.C1 * gm.C1_INV) % (1 << 32) == 1 and (gm.C2 * gm.C2_INV) % (1 << 32) == 1
    x = np.random.default_rng(1).integers(0, 1 << 32, 10 ** 6, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(gm.mix32_inverse(gm.mix32(x)), x)
    assert np.array_equal(gm.mix32(gm.mix32_inverse(x)), x)
    # a few fixed values of lowbias32, worked by hand from its definition with Python integers
    for v in (0, 1, 0xFFFFFFFF, 0x12345678):
        y = v
        y ^= y >> 16
        y = (y * gm.C1) & gm.M32
        y ^= y >> 15
        y = (y * gm.C2) & gm.M32
        y ^= y >> 16
        assert int(gm.mix32(v)) == y


@pytest.mark.parametrize("keys", KEYS)
def test_uniform_ranges(keys):
    k0, k1 = keys
    idx = np.random.default_rng(2).integers(0, 1 << 32, 10 ** 6, dtype=np.uint64).astype(np.uint32)
    u1, u2 = gm.uniforms(k0, k1, idx)
    assert u1.min() > 0.0 and u1.max() <= 1.0 and u2.min() >= 0.0 and u2.max() < 1.0
    assert np.array_equal(u1, u1.astype(np.float32)) and np.array_equal(u2, u2.astype(np.float32))       # exact in float32
    # the extreme hash words, reached through the inverse: a = 0 gives the smallest u1 and u2 = 0, a = 2^32 - 1 gives u1 = 1
    lo = gm.uniforms(k0, k1, idx_for_word(k0, k1, 0))
    hi = gm.uniforms(k0, k1, idx_for_word(k0, k1, 0xFFFFFFFF))
    assert float(lo[0]) == 2.0 ** -16 and float(lo[1]) == 0.0
    assert float(hi[0]) == 1.0 and float(hi[1]) == 1.0 - 2.0 ** -16
    zmax = math.sqrt(2.0 * math.log(65536.0))
    assert float(gm.box_muller(*lo)) == pytest.approx(zmax, abs=1e-15) and float(gm.box_muller(*hi)) == 0.0
    assert np.abs(gm.box_muller(u1, u2)).max() <= zmax


def test_grid_is_the_law_of_a_full_cycle():
    """mix32 is a bijection, so as idx runs over all 2^32 words the hash word a does too, and (u1, u2) visits every point of
    the 65536 x 65536 grid once.  The grid's moments in closed form; its largest |z| is sqrt(2 ln 65536)."""
    m1, var, m4 = grid_moments()
    assert abs(m1) < 1e-12                                    # the angles sum to zero
    assert 0.9997 < var < 1.0                                 # E[-2 ln u1] / 2 on the grid: 1 - O(16 / 65536)
    assert 2.99 < m4 < 3.0
    assert max(abs(v) for v in (gm.box_muller(2.0 ** -16, 0.0), gm.box_muller(1.0, 0.0))) == pytest.approx(math.sqrt(2.0 * math.log(N16)))


@pytest.mark.parametrize("seed,frame", [((1 << 64) - 1, (1 << 32) + 1), (0x243F6A8885A308D3, 7)])
def test_4k_plane_matches_the_grid_law(seed, frame):
    """A 4K plane is 8.3 M distinct words of the cycle: its mean and variance against the grid's at 5 sigma."""
    h, w = 2160, 3840
    z, u1 = gm.plane(seed, frame, h, w, with_u1=True)
    m1, var, m4 = grid_moments()
    n = z.size
    assert abs(z.mean() - m1) < 5.0 * math.sqrt(var / n), (z.mean(), m1)
    assert abs(z.var() - var) < 5.0 * math.sqrt((m4 - var * var) / n), (z.var(), var)
    assert u1.min() > 0.0 and u1.max() <= 1.0
    assert np.array_equal(z == 0.0, u1 == 1.0)


def test_plane_index_is_row_major():
    z = gm.plane(5, 6, 7, 65)
    k0, k1 = gm.noise_keys(5, 6)
    y, x = 4, 63
    assert z[y, x] == float(gm.box_muller(*gm.uniforms(k0, k1, np.uint32(y * 65 + x))))
    assert np.array_equal(z.ravel(), gm.plane(5, 6, 1, 7 * 65).ravel())
    assert [p.shape for p in gm.planes(5, 6, 2, 9, 20, grain_size=2)] == [(4, 10)] * 2
    assert [p.shape for p in gm.planes(5, 6, 1, 1, 1, grain_size=3)] == [(1, 1)]


def test_keys_take_the_high_half_of_the_seed():
    for s0 in (0, 1, 99, 0xFFFFFFFF, 0x85A308D3):
        keys = {gm.noise_keys((s1 << 32) | s0, f) for s1 in (0, 1, 0x80000000, 0xFFFFFFFF) for f in (0, 1 << 32)}
        assert len(keys) == 8, s0


def test_keys_take_the_high_half_of_the_frame_index():
    for seed in (0, 99, 1 << 63, (1 << 64) - 1):
        keys = [gm.noise_keys(seed, f) for f in ((1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1, (1 << 33) + 1, (1 << 63) + 1)]
        assert len(set(keys)) == len(keys), seed


def test_no_key_collisions_around_the_word_boundaries():
    seeds = [b + d for b in (0, 1 << 32, 1 << 63, (1 << 64) - 16) for d in range(16)]
    frames = [b + d for b in (0, (1 << 32) - 8, (1 << 33) - 8) for d in range(16)]
    keys = {gm.noise_keys(s, f) for s in seeds for f in frames}
    assert len(keys) == len(seeds) * len(frames)


def test_keys_reject_out_of_range():
    for s, f in ((-1, 0), (1 << 64, 0), (0, -1), (0, 1 << 64)):
        with pytest.raises(ValueError):
            gm.noise_keys(s, f)
