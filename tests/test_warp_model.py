"""tests/warp_model.py (the float32-storage model the GPU warp / commit kernels are held to bit for bit) against the unmodified oracle, and
the census that shows the geometry set of the GPU sweep is not vacuous.  CPU only.

The model is the oracle with two float32 roundings inserted (the stored pre-warp image, the stored persistence state).  It must therefore
lie within the bars DESIGN.md §5 states for the warp — and those bars are asserted here as they stand: warped float image 3e-7, uint8 frame
1 LSB on < 0.1 % of the samples, half frames one half ulp on < 0.5 %, persistence states 4e-7.  An unpromoted chain is float32 from end to
end in the reference too, so there the model IS the oracle and the comparison is an equality."""
import numpy as np
import pytest

from oracle import crt_oracle as orc
from tests import warp_model as wm

CHAINS = {"unpromoted": wm.OFF, "promoted": wm.FULL}


def half_ulp(x):
    """Spacing of float16 at |x| (normal range; the frames here lie in [0, 255])."""
    x = np.maximum(np.abs(x.astype(np.float32)), np.float32(2.0 ** -14))
    return np.exp2(np.floor(np.log2(x)) - 10.0)


@pytest.mark.parametrize("chain", sorted(CHAINS))
@pytest.mark.parametrize("s", wm.STRENGTHS)
def test_model_within_the_oracle_bars(chain, s):
    """Static float image, 5-frame persistence chain (states, uint8 and half quantisation of them) on every shape of the sweep."""
    n_u8 = bad_u8 = n_h = bad_h = 0
    for k, (h, w) in enumerate(wm.SHAPES):
        cfg = dict(CHAINS[chain], warp_strength=s, persistence=0.5)
        frames = [wm.make_frame(h, w, 100 * k + j) for j in range(5)]
        planes = [wm.make_plane(h, w, 7000 + 100 * k + j) for j in range(5)] if cfg["noise_strength"] > 0 else None
        outs, states = wm.oracle_render(frames, cfg, first=3, planes=planes)
        m_outs, m_states = wm.render(frames, cfg, first=3, planes=planes)
        # the static image of the first frame (the first frame of a chain passes through unblended)
        pre = wm.pre_images(frames[:1], cfg, first=3, planes=None if planes is None else planes[:1])[0]
        assert np.array_equal(wm.static_image(pre, s), m_states[0])
        assert np.abs(m_states[0].astype(np.float64) - states[0]).max() <= 3e-7, (h, w)
        for j in range(5):
            assert m_states[j].dtype == np.float32
            assert states[j].dtype == (np.float64 if chain == "promoted" else np.float32)
            assert np.abs(m_states[j].astype(np.float64) - states[j]).max() <= 4e-7, (h, w, j)
            d = np.abs(m_outs[j].astype(np.int16) - outs[j].astype(np.int16))
            assert d.max() <= 1, (h, w, j)
            n_u8 += d.size
            bad_u8 += int((d != 0).sum())
            exp16 = np.abs(states[j].astype(np.float32) * np.float32(255.0)).astype(np.float16)
            got16 = wm.to_half(m_states[j])
            assert np.all(np.abs(got16.astype(np.float32) - exp16.astype(np.float32)) <= half_ulp(exp16)), (h, w, j)
            n_h += got16.size
            bad_h += int((got16 != exp16).sum())
            if chain == "unpromoted":
                assert np.array_equal(m_states[j], states[j]) and np.array_equal(m_outs[j], outs[j]), (h, w, j)
    assert bad_u8 / n_u8 < 1e-3, (bad_u8, n_u8)
    assert bad_h / n_h < 5e-3, (bad_h, n_h)


@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_preview_commit_within_the_oracle_bars(chain):
    """apply_crt_effect's addWeighted blend over 4 ticks, with the warp and a glitch band."""
    h, w = 70, 130
    cfg = dict(CHAINS[chain], warp_strength=0.15)
    tm = orc.make_triad_mask(h, w, cfg["triad_strength"], cfg["triad_softness"]) if cfg["triad_strength"] > 0 else None
    vg = orc.make_vignette(h, w, cfg["vignette_strength"]) if cfg["vignette_strength"] > 0 else None
    so = sm = None
    for i in range(4):
        frame = wm.make_frame(h, w, 40 + i)
        plane = wm.make_plane(h, w, 50 + i) if cfg["noise_strength"] > 0 else None
        a = (frame, cfg["scanline_strength"], tm, 2.2, False, cfg["aberration_px"], cfg["bloom_sigma"], cfg["bloom_strength"], 0.0,
             cfg["noise_strength"], vg, 0.5, so, 2.0, float(i), False, 1, 6, 0.25)
        uo, so = orc.apply_crt_effect(*a, warp_strength=0.15, noise_plane=plane)
        pre = orc.apply_static_effects(*(a[:11] + a[13:17]), 0, 0.0, noise_plane=plane, stop_before_warp=True)
        pre = pre.astype(np.float32).astype(pre.dtype)
        um, sm = wm.preview_step(wm.warp(pre, 0.15, orc.glitch_offsets_preview(h, w, float(i), 6, 0.25)), 0.5, sm)
        assert np.abs(sm.astype(np.float64) - so).max() <= 4e-7
        d = np.abs(um.astype(np.int16) - uo.astype(np.int16))
        assert d.max() <= 1 and (d != 0).mean() < 1e-3


def test_model_is_the_same_under_both_remap_summation_forms():
    """In float64 the products of float32-valued taps and float32 weights are exact, so OpenCV's contracted sum (VARIANT["remap_fma"]) gives
    the model the same bits: the kernels' fma chain (wsum4) is not a choice between variants."""
    h, w = 37, 129
    pre = wm.pre_images([wm.make_frame(h, w, 5)], dict(wm.FULL, noise_strength=0.0))[0]
    assert pre.dtype == np.float64
    for s in wm.STRENGTHS:
        a = wm.warp(pre, s)
        with orc.opencv_variant(remap_fma=1):
            b = wm.warp(pre, s)
        assert np.array_equal(a, b), s


def test_census_reproduces_a_hand_count():
    c = wm.census(33, 65, 0.15)
    assert [c[k] for k in wm.CLASSES] == [1716, 46, 105, 4, 274, 26, 127], c


@pytest.mark.parametrize("s", [s for s in wm.STRENGTHS if s >= 0.15])
def test_every_tap_class_is_populated(s):
    """For each outward strength at least one shape of the sweep has pixels of every class, the two clamped ranges included."""
    best = {k: 0 for k in wm.CLASSES}
    for h, w in wm.SHAPES:
        for k, v in wm.census(h, w, s).items():
            best[k] = max(best[k], v)
    assert all(v > 0 for v in best.values()), (s, best)


@pytest.mark.parametrize("s", [-0.4, -1.0])
def test_inward_strengths_are_all_in(s):
    """A negative strength pulls every tap inside (apart from the zero-weight right / bottom tap of the last column / row)."""
    for h, w in wm.SHAPES:
        ix, iy, fxy = orc.remap_quantise(*orc.barrel_maps(h, w, s))
        assert ix.min() >= 0 and iy.min() >= 0 and ix.max() <= w - 1 and iy.max() <= h - 1, (h, w)
        assert np.all((fxy & 31)[ix == w - 1] == 0) and np.all((fxy >> 5)[iy == h - 1] == 0), (h, w)


@pytest.mark.parametrize("s", [1e-3, -1e-3])
def test_tiny_strengths_sit_on_zero_fractions(s):
    """+-1e-3 leaves a large share of the pixels on a fraction of exactly 0 and masks the right / bottom edge taps only."""
    shares = [wm.zero_fraction_share(h, w, s) for h, w in wm.SHAPES if h * w > 1]
    assert min(shares) >= 0.10 and max(shares) <= 1.0, shares
    for h, w in wm.SHAPES:
        ix, iy, _ = orc.remap_quantise(*orc.barrel_maps(h, w, s))
        assert ix.min() >= -1 and iy.min() >= -1 and ix.max() <= w - 1 and iy.max() <= h - 1, (h, w)
