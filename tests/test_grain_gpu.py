"""GPU: the in-kernel film grain (stage a11) against the host model of its generator (tests/grain_model.py).

Every other render test that has grain on feeds the oracle the plane crtfx_noise_plane exports, and that plane comes from the
same grain_normal, with keys from the same noise_keys, as the render kernels' draw: an error in either would move both sides at
once.  Here the reference is the float64 numpy model instead:
  * a — crtfx_noise_plane pixel by pixel against grain_model.plane, seeds and frame indices over both 32-bit halves;
  * b — each kernel build that draws grain in-kernel (pinned through its plan string) against the oracle fed grain_model's
        planes, never the exported ones.  Bars are the ones the existing tests use for each family."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import crt_oracle as orc  # noqa: E402  (checker only)
from tests import grain_model as gm  # noqa: E402

# ---- a: the exported plane -----------------------------------------------------------------------------------------------------

SEEDS = [0, 1, 99, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 1, 0xC0FFEE1234ABCDEF]
FRAMES = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 33) + 5]
# |z_gpu - z_model| at every pixel.  The kernel's log2 / sqrt / cos are the hardware v_log_f32 / v_sqrt_f32 / v_cos_f32; on an
# MI355X the largest error over the 126 planes below was 9.25e-7 (|z| = 4.27, two float32 ulps there).  EPS leaves a 2x margin.
EPS = 2e-6


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device("cuda", torch.cuda.current_device())


def gpu_plane(eng, seed, frame):
    out = torch.empty((eng.h, eng.w), dtype=torch.float32, device=eng.device)
    assert eng.lib.crtfx_noise_plane(eng.ctx, seed, frame, out.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    return out.cpu().numpy()


def plane_error(got, seed, frame):
    """Checks the exported plane against the model; returns max |z_gpu - z_model|."""
    h, w = got.shape
    want, u1 = gm.plane(seed, frame, h, w, with_u1=True)
    err = np.abs(got.astype(np.float64) - want)
    where = np.unravel_index(int(err.argmax()), err.shape)
    assert err.max() <= EPS, (seed, frame, float(err.max()), where, float(got[where]), float(want[where]))
    assert np.all(got[u1 == 1.0] == 0.0), (seed, frame)                     # u1 = 1: radius exactly 0
    big = np.abs(want) > EPS
    assert np.array_equal(np.sign(got[big]), np.sign(want[big])), (seed, frame)
    return float(err.max())


@pytest.mark.parametrize("hw", [(1, 1), (7, 65), (33, 641)])
def test_noise_plane_matches_the_model(dev, hw):
    """Every seed crossed with every frame index."""
    from pythoncrt_amd.effects import Engine
    eng = Engine(dev, *hw)
    for seed in SEEDS:
        for frame in FRAMES:
            plane_error(gpu_plane(eng, seed, frame), seed, frame)


@pytest.mark.parametrize("hw,seed,frame", [((1080, 1920), (1 << 64) - 1, 1 << 32), ((1080, 1920), 1 << 63, 1), ((1080, 1920), 0, (1 << 33) + 5),
                                           ((2160, 3840), 0xC0FFEE1234ABCDEF, (1 << 32) - 1), ((2160, 3840), 1 << 32, 0),
                                           ((2160, 3840), (1 << 64) - 1, (1 << 33) + 5)])
def test_noise_plane_matches_the_model_full_size(dev, hw, seed, frame):
    from pythoncrt_amd.effects import Engine
    got = gpu_plane(Engine(dev, *hw), seed, frame)
    _, u1 = gm.plane(seed, frame, *hw, with_u1=True)
    assert (u1 == 1.0).any()                                                 # the u1 = 1 check is not vacuous at these sizes
    plane_error(got, seed, frame)


# ---- b: every in-kernel draw, through the oracle ---------------------------------------------------------------------------------

FPS = 25.0
PARAM_KEYS = ("scanline_strength", "triad_gamma", "triad_preserve_luma", "aberration_px", "bloom_sigma", "bloom_strength", "bloom_threshold",
              "noise_strength", "scanline_period_px", "fast_bloom", "pixel_size", "glitch_amp_px", "glitch_height_frac", "brightness", "contrast",
              "gamma", "saturation", "temperature", "flicker_strength", "flicker_hz", "grain_size", "scanline_angle", "scanline_thickness",
              "warp_strength")
WRAP = (1 << 32) - 2            # a batch from here straddles the wrap of the frame index's low 32 bits
HI_SEED, TOP_SEED = (1 << 63) + 0x5DEECE66D, (1 << 64) - 1


def settings(base, **kw):
    from pythoncrt_amd.pipeline import RenderSettings, baseline_config
    rs = RenderSettings() if base == "cli" else baseline_config(2)[0]       # the reference CLI's defaults / BASELINE config 2's full chain
    return dataclasses.replace(rs, **kw)


# id: (settings base, overrides, (h, w), frames, first index, seed, half frames, debug options, plan key, plan value).  Every seed has a
# non-zero high half, so that a build which lost it fails here.
RENDER_CASES = {
    "fused": ("cli", dict(noise_strength=4.0), (90, 326), 4, 0, TOP_SEED, False, {},
              "point", "k_point_fused_seq<fast+pixelate,u8,render>"),
    "fused_coarse": ("cli", dict(noise_strength=5.0, grain_size=2), (90, 326), 4, WRAP, HI_SEED, False, {},
                     "point", "k_point_fused_seq<fast+pixelate+coarse,u8,render>"),
    "sel_seq_coarse": ("cli", dict(noise_strength=4.0, grain_size=2, saturation=1.4), (37, 130), 4, 7, (99 << 32) + 99, False, {},
                       "point", "k_point_sel_seq<u8,two-round>"),
    "lean_seq": ("cli", dict(noise_strength=6.0), (90, 326), 4, 3, 1 << 32, False, {"NO_FUSED_HALF": 1},
                 "point", "k_point_lean_seq<fast+pixelate,u8,render>"),
    "runtime_flags": ("cli", dict(noise_strength=4.0), (90, 326), 4, 1 << 32, (1 << 40) + 12345, False, {"FORCE_RUNTIME_FLAGS": 1},
                      "point", "k_point_sel_seq<u8,two-round>"),
    "point_generic": ("cli", dict(noise_strength=4.0), (33, 641), 3, 1, 0xC0FFEE1234ABCDEF, False, {"FORCE_GENERIC": 1},
                      "point", "k_point<runtime>"),
    "ct_u8_r4": ("full", dict(noise_strength=4.0, warp_strength=0.0, persistence=0.5), (44, 641), 4, WRAP, 1 << 63, False, {},
                 "phosphor", "k_phosphor_ct<4,u8>"),
    "ct_u8_r9": ("full", dict(noise_strength=6.0, bloom_sigma=3.0), (90, 326), 4, 11, TOP_SEED, False, {},
                 "phosphor", "k_phosphor_ct<9,u8>"),
    "ct_half_r9": ("full", dict(noise_strength=4.0, bloom_sigma=3.0, warp_strength=0.0, persistence=0.5), (44, 641), 3, WRAP, (7 << 32) + 7, True, {},
                   "phosphor", "k_phosphor_ct<9,half>"),
    "ct_half_r4": ("full", dict(noise_strength=5.0), (90, 326), 3, 5, HI_SEED, True, {},
                   "phosphor", "k_phosphor_ct<4,half>"),
    "rr": ("full", dict(noise_strength=4.0, warp_strength=0.0, persistence=0.3), (44, 641), 4, 2, 1 << 32, False, {"NO_CT": 1},
           "phosphor", "k_phosphor_rr<4,full,u8>"),
    "rr_coarse": ("full", dict(noise_strength=6.0, warp_strength=0.0, persistence=0.3, grain_size=3), (44, 641), 4, 9, 0xFFFFFFFF00000000, False, {},
                  "phosphor", "k_phosphor_rr<4,runtime,u8>"),
    "cc": ("full", dict(noise_strength=4.0), (44, 641), 4, 1 << 32, (1 << 32) + 1, False, {"FORCE_CC": 1, "NO_CT": 1},
           "phosphor", "k_phosphor_cc<4,u8>"),
    "phosphor_generic": ("full", dict(noise_strength=5.0, warp_strength=0.0, persistence=0.3), (44, 641), 3, 0, 0xC0FFEE1234ABCDEF, False, {"FORCE_GENERIC": 1},
                         "phosphor", "k_phosphor<-1>"),
}


@pytest.fixture
def debug_options(monkeypatch):
    from pythoncrt_amd import effects

    def use(opts):
        monkeypatch.setattr(effects, "DEBUG_OPTIONS", dict(opts))
        effects._tls.engines = {}
    yield use
    effects._tls.engines = {}


@pytest.mark.parametrize("case", list(RENDER_CASES))
def test_in_kernel_grain_matches_the_model(dev, debug_options, case):
    """FramePipeline.run (in-kernel draw) against the oracle fed grain_model's planes.  u8: <= 1 LSB on < 1e-3 of the samples;
    half: <= 0.125 on < 5e-3 (the sweep's bar); persistence state <= 1e-6."""
    from pythoncrt_amd.pipeline import FramePipeline
    base, kw, (h, w), n, first, seed, half, opts, key, want = RENDER_CASES[case]
    rs = settings(base, **kw)
    debug_options(opts)
    rng = np.random.default_rng(len(case) * 1000 + h + w)
    if half:
        frames = (rng.random((n, h, w, 3), dtype=np.float32) * 255.0).astype(np.float16)
    else:
        frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    pipe = FramePipeline(dev, h, w, rs, fps=FPS, noise_seed=seed, dtype=torch.float16 if half else torch.uint8)
    out, state = pipe.run(torch.from_numpy(frames).to(dev), first_index=first)
    plan = pipe.plan()
    got = out.cpu().numpy()
    planes = gm.planes(seed, first, n, h, w, rs.grain_size)
    params = {k: getattr(rs, k) for k in PARAM_KEYS}
    masks = (rs.triad_strength, rs.triad_softness, rs.vignette_strength)
    if half:
        st = None
        for i in range(n):
            _, st = orc.process_frames([frames[i]], params, FPS, rs.scanline_speed_px_s, rs.persistence, *masks,
                                       noise_planes=[planes[i]], first_index=first + i, prev_state=st)
            exp16 = np.abs(st.astype(np.float32) * np.float32(255.0)).astype(np.float16)
            diff = np.abs(got[i].astype(np.float32) - exp16.astype(np.float32))
            assert diff.max() <= 0.125 and (got[i] != exp16).mean() < 5e-3, (case, i, float(diff.max()), float((got[i] != exp16).mean()))
            if rs.persistence <= 0.0:
                st = None
        exp_state = st
    else:
        exp, exp_state = orc.process_frames(list(frames), params, FPS, rs.scanline_speed_px_s, rs.persistence, *masks,
                                            noise_planes=planes, first_index=first)
        d = np.abs(got.astype(np.int16) - np.stack(exp).astype(np.int16))
        assert d.max() <= 1 and (d != 0).mean() < 1e-3, (case, int(d.max()), float((d != 0).mean()))
    if rs.persistence > 0.0:
        assert np.abs(state.cpu().numpy().astype(np.float64) - exp_state).max() <= 1e-6, case
    assert plan.get(key) == want, (case, plan)


# the single-frame path: apply_static_effects(..., noise_seed=, frame_index=) -> crtfx_apply_static
STATIC_CASES = {
    "fast_bloom": (dict(pixel_size=2, fast_bloom=True, bloom_sigma=1.2, noise_strength=6.0), (45, 130), TOP_SEED, (1 << 32) + 1,
                   "point", "k_point_sel<u8,two-round>"),
    "gauss_bloom": (dict(pixel_size=1, fast_bloom=False, bloom_sigma=3.0, noise_strength=5.0), (44, 641), HI_SEED, (1 << 32) - 1,
                    "phosphor", "k_phosphor_rr<9,full,u8>"),
    "coarse": (dict(pixel_size=1, fast_bloom=False, bloom_sigma=1.2, noise_strength=4.0, grain_size=3), (37, 130), 1 << 63, 1 << 33,
               "phosphor", "k_phosphor_rr<4,runtime,u8>"),
}


@pytest.mark.parametrize("case", list(STATIC_CASES))
def test_single_frame_grain_matches_the_model(dev, debug_options, case):
    """The float image of one frame, drawn in-kernel from (noise_seed, frame_index), against the oracle fed the model's plane:
    <= 1e-6 absolute (the grain alone moves a pixel by noise_strength / 255 * |z|, some 1e-2)."""
    import pythoncrt_amd as pc
    kw, (h, w), seed, frame_index, key, want = STATIC_CASES[case]
    debug_options({})
    img = np.random.default_rng(h * w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    c = dict(dict(scanline_strength=0.6, triad_gamma=2.2, triad_preserve_luma=False, aberration_px=1, bloom_strength=0.25, bloom_threshold=0.0,
                  scanline_period_px=2.0, scanline_phase_px=1.25), **kw)
    grain = int(c.pop("grain_size", 1))

    def args(mod):
        return (img, c["scanline_strength"], mod.make_triad_mask(h, w, 0.35, 0.5), c["triad_gamma"], c["triad_preserve_luma"], c["aberration_px"],
                c["bloom_sigma"], c["bloom_strength"], c["bloom_threshold"], c["noise_strength"], mod.make_vignette(h, w, 0.25),
                c["scanline_period_px"], c["scanline_phase_px"], c["fast_bloom"], c["pixel_size"], 0, 0.0)
    got = pc.apply_static_effects(*args(pc), grain_size=grain, noise_seed=seed, frame_index=frame_index)
    plan = pc.effects._engine(dev, h, w).last_plan()
    plane = gm.planes(seed, frame_index, 1, h, w, grain)[0]
    exp = orc.apply_static_effects(*args(orc), grain_size=grain, noise_plane=plane)
    err = np.abs(got.astype(np.float64) - exp)
    assert err.max() <= 1e-6, (case, float(err.max()))
    assert plan.get(key) == want, (case, plan)
