"""Every per-radius k_phosphor build held to the oracle, bit for bit, with in-kernel grain.

libcrtfx.so compiles crtfx_rr.hip once per bloom radius 1 .. 30 and each build instantiates up to eight launch variants: 150 k_phosphor_rr,
30 k_phosphor_cc and 30 k_phosphor_ct, plus the generic LDS-ring k_phosphor<-1> that takes the radius at run time.  Much of their code
changes with R itself (k_phosphor_ct's ring shift R % NB, the odd/even tap pairing at t == 2R + 1, the half build's packed register window
of (R + NB + 1) / 2 VGPRs, the LDS strides rr_pad(R) / cc_sws(R), the pixelate build's seg_rows + 2R LDS rows), so a mistake shows at some
radii only.  The table tests/radius_builds.BUILDS names every build and how it is reached; this file runs each row at each of its radii
(sigma = R / 3) on shapes chosen relative to R, checks that crtfx_last_plan names exactly that build (a planner fallback fails here instead
of passing against another kernel), and compares against the oracle fed with the grain planes the library drew (crtfx_noise_plane):

  * short:   fewer rows than R, one partial strip of an odd width (the border reflection wraps more than once);
  * halo:    W = 2 * TW + R + 3 (the last strip is partial, the horizontal halo crosses strip boundaries), H % NB != 0;
  * segment: a taller frame with SEG_ROWS = 8, every block's rows shorter than its 2R halo (k_phosphor<-1>: the planner's segments).

Bars, none loosened:
  * `api` rows (apply_static_effects, no warp, no gamma): the float image, float32(oracle) == gpu;
  * `loop` rows (FramePipeline.run, 3 frames with GROUP = 3 — one launch on the halo and segment shapes; the short shapes run their
    frames one launch each, and k_phosphor_ct's short shapes only one frame, see loop_frames — persistence on and no warp, so the
    column-owner kernels park a pre-warp image and the per-frame states are that image blended): frame 0 passes through unblended, so its state is compared bit for
    bit and its uint8 frame is bit-exact; blended uint8 frames are <= 1 LSB off on < 1e-3 of the samples; half frames keep
    test_fp16_frames' bars (<= 0.125, < 5e-3 of the samples off).  On the short shape the persistence is 1e-300: the blend is then the
    identity in float64 (and in float32), so every frame's state is its pre-warp image and is compared bit for bit — a shape of a few
    hundred samples cannot carry a 1e-3 rate of one-LSB flips.

A second part walks the split path (k_sb_rows + k_sb_cols_lds / k_sb_cols<4|1>) across the radii where its shape changes."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import crt_oracle as orc  # noqa: E402  (checker only)
from tests import radius_builds as rb  # noqa: E402

SEED = 4099
FIRST = 3                   # frame index of the first frame (grain and scanline phase)
TINY_PERSISTENCE = 1e-300   # blend on (a pre-warp image is parked), but p * prev vanishes next to any non-zero pixel


def ab_for(R):
    """A non-zero aberration whose sign alternates with R (ref:1230 allows -8 .. 8)."""
    return (1 + R % 4) * (1 if R % 2 else -1)


def ragged_height(h, w):
    """The first height from h on with H % NB != 0 whose frames, packed one after the other, all start on an 8-byte boundary (k_phosphor_ct
    reads a frame row as aligned dwords / qwords; a frame that does not start on one takes k_phosphor_cc / k_phosphor_rr, same bits)."""
    while h % rb.NB == 0 or (h * w) % 4:
        h += 1
    return h


def shapes(build, R):
    """[(label, h, w, extra options)] of one case."""
    w_halo = 2 * rb.TW + R + 3
    out = [("short", max(1, R // 2), 37, {}),
           ("halo", ragged_height(max(2 * R + 13, GROUP_MIN_ROWS), w_halo), w_halo, {})]
    if build.family == "k_phosphor":
        out.append(("segment", ragged_height(4 * R + 37, 70), 70, {}))
    else:
        out.append(("segment", ragged_height(4 * R + 37, 70), 70, {"SEG_ROWS": 8}))
    return out


# plan_grid only weighs row segments of 24 rows and more (crtfx.hip): a frame of at most 16 rows (24 rounded down to NB) has no
# candidate and keeps one frame per launch whatever CRTFX_OPT_GROUP asks for.  The halo and segment shapes are at least this tall, so every
# loop row runs its GROUP = 3 launch; the short shapes (fewer rows than R <= 30) run their frames one launch each.
GROUP_MIN_ROWS = 17


def expected_group(n, h):
    return n if h >= GROUP_MIN_ROWS else 1


def loop_frames(build, h, w):
    """Frames per render-loop run: 3 (one GROUP = 3 launch), or 1 where a packed batch would put frames 1 and 2 off the alignment
    k_phosphor_ct loads with (the short shapes: fewer rows than R, an odd width) and the launch would rightly land on another build."""
    align = 8 if build.pix == "half" else 4
    return 3 if build.family != "k_phosphor_ct" or (h * w * 3 * (2 if build.pix == "half" else 1)) % align == 0 else 1


def cases():
    out = []
    for b in rb.BUILDS:
        for R in b.radii:
            out.append(pytest.param(b.name, R, id=f"{b.name}-R{R}"))
    return out


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    import pythoncrt_amd
    from pythoncrt_amd import effects
    saved = effects.DEBUG_OPTIONS
    state = {"opts": None}
    yield pythoncrt_amd, effects, state
    effects.DEBUG_OPTIONS = saved
    effects._tls.engines = {}
    torch.cuda.empty_cache()


def use_options(env, opts):
    """Hand `opts` to every ctx created from now on; the cached engines are dropped only when the options change."""
    _, effects, state = env
    key = tuple(sorted(opts.items()))
    if state["opts"] != key:
        effects.DEBUG_OPTIONS = dict(opts)
        effects._tls.engines = {}
        state["opts"] = key


def make_frame(h, w, seed, half):
    rng = np.random.default_rng(seed)
    if half:
        return (rng.random((h, w, 3), dtype=np.float32) * 255.0).astype(np.float16)      # fractional values on the 0..255 scale
    yy, xx = np.mgrid[0:h, 0:w]
    g = np.stack([(xx * 255) // max(1, w - 1), (yy * 255) // max(1, h - 1), ((xx + yy) * 255) // max(1, h + w - 2)], axis=2)
    return np.clip((g + rng.integers(0, 64, (h, w, 3))) // 2 + 40 + rng.integers(-40, 40, (h, w, 3)), 0, 255).astype(np.uint8)


def export_plane(lib, ctx, h, w, index):
    p = torch.empty((h, w), dtype=torch.float32, device=torch.device("cuda", torch.cuda.current_device()))
    assert lib.crtfx_noise_plane(ctx, SEED, index, p.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    return p.cpu().numpy()


def assert_bit_exact(got, exp, what):
    e32 = np.asarray(exp).astype(np.float32)
    got = np.asarray(got)
    if not np.array_equal(got, e32):
        d = np.abs(got.astype(np.float64) - e32)
        bad = np.argwhere(got != e32)
        raise AssertionError(f"{what}: {(got != e32).sum()} of {got.size} differ; max |d| = {d.max():.3e}; first at {bad[0].tolist()}")


def static_args(frame, R, tm, vg, thr, px):
    s = rb.FULL
    return (frame, s["scanline_strength"], tm, 2.2, False, ab_for(R), R / 3.0, s["bloom_strength"], thr, s["noise_strength"], vg,
            2.0, 1.25, False, px, 0, 0.0)


def run_api(env, build, R, h, w, opts, px=1, sigma=None, seed=0):
    """One frame through apply_static_effects: -> (plan, gpu float image, oracle float image)."""
    pc, effects, _ = env
    use_options(env, opts)
    half = build.pix == "half"
    frame = make_frame(h, w, 1000 * R + seed, half)
    thr = build.settings.get("bloom_threshold", 0.0)
    tri, vig = rb.FULL["triad"], rb.FULL["vignette"]
    a_g = list(static_args(frame, R, pc.make_triad_mask(h, w, *tri), pc.make_vignette(h, w, vig), thr, px))
    a_o = list(static_args(frame, R, orc.make_triad_mask(h, w, *tri), orc.make_vignette(h, w, vig), thr, px))
    if sigma is not None:
        a_g[6] = a_o[6] = sigma
    got = pc.apply_static_effects(*a_g, noise_seed=SEED, frame_index=FIRST)
    from pythoncrt_amd import _lib
    eng = effects._engine(torch.device("cuda", torch.cuda.current_device()), h, w, _lib.PIX_F16 if half else _lib.PIX_U8)
    plan = eng.last_plan()
    plane = export_plane(eng.lib, eng.ctx, h, w, FIRST)
    exp = orc.apply_static_effects(*a_o, noise_plane=plane)
    return plan, got, exp


def oracle_states(frames, rs, planes):
    """The oracle's in-order render, one frame at a time: per-frame float states (float64) and uint8 frames."""
    params = {k: getattr(rs, k) for k in ("scanline_strength", "triad_gamma", "triad_preserve_luma", "aberration_px", "bloom_sigma",
                                          "bloom_strength", "bloom_threshold", "noise_strength", "scanline_period_px", "fast_bloom",
                                          "pixel_size", "warp_strength")}
    states, outs, st = [], [], None
    for j, f in enumerate(frames):
        o, st = orc.process_frames([f], params, 30.0, rs.scanline_speed_px_s, rs.persistence, rs.triad_strength, rs.triad_softness,
                                   rs.vignette_strength, noise_planes=[planes[j]], first_index=FIRST + j, prev_state=st)
        states.append(st)
        outs.append(o[0])
    return states, outs


def run_loop(env, build, R, h, w, opts, persistence):
    """loop_frames() frames through FramePipeline.run with GROUP = 3; checks the plan and the bars."""
    _, effects, _ = env
    from pythoncrt_amd.pipeline import FramePipeline, RenderSettings
    half = build.pix == "half"
    saved = effects.DEBUG_OPTIONS
    effects.DEBUG_OPTIONS = dict(opts, GROUP=3)      # FramePipeline makes its own ctx: nothing cached to drop
    dev = torch.device("cuda", torch.cuda.current_device())
    rs = RenderSettings(scanline_strength=rb.FULL["scanline_strength"], triad_strength=rb.FULL["triad"][0], triad_softness=rb.FULL["triad"][1],
                        triad_gamma=2.2, aberration_px=ab_for(R), bloom_sigma=R / 3.0, bloom_strength=rb.FULL["bloom_strength"],
                        bloom_threshold=0.0, noise_strength=rb.FULL["noise_strength"], vignette_strength=rb.FULL["vignette"],
                        persistence=persistence, fast_bloom=False, pixel_size=1, warp_strength=0.0)
    n = loop_frames(build, h, w)
    frames = np.stack([make_frame(h, w, 1000 * R + 7 * j + 3, half) for j in range(n)])
    pipe = FramePipeline(dev, h, w, rs, fps=30.0, noise_seed=SEED, dtype=torch.float16 if half else torch.uint8)
    local = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev)
    out, _ = pipe.run(torch.from_numpy(frames).to(dev), first_index=FIRST, local_states=local)
    plan = pipe.plan()
    planes = [export_plane(pipe.lib, pipe.engine.ctx, h, w, FIRST + j) for j in range(n)]
    out, local = out.cpu().numpy(), local.cpu().numpy()
    del pipe
    effects.DEBUG_OPTIONS = saved
    assert plan.get("phosphor") == build.plan_for(R) and plan.get("group") == expected_group(n, h), plan
    states, outs = oracle_states(list(frames), rs, planes)
    exact = range(n) if persistence == TINY_PERSISTENCE else range(1)
    for j in exact:
        assert_bit_exact(local[j], states[j], f"state of frame {j}")
    if half:
        exp16 = np.stack([np.abs(s.astype(np.float32) * np.float32(255.0)).astype(np.float16) for s in states])
        for j in exact:
            assert np.array_equal(out[j], exp16[j]), f"half frame {j}: {(out[j] != exp16[j]).sum()} samples differ"
        assert np.abs(out.astype(np.float32) - exp16.astype(np.float32)).max() <= 0.125, "half frame off by more than one half ulp"
        assert (out != exp16).mean() < 5e-3
    else:
        exp = np.stack(outs)
        for j in exact:
            assert np.array_equal(out[j], exp[j]), f"uint8 frame {j}: {(out[j] != exp[j]).sum()} samples differ"
        if n > 1:
            d = np.abs(out[1:].astype(np.int16) - exp[1:].astype(np.int16))
            assert d.max() <= 1 and (d != 0).mean() < 1e-3, (int(d.max()), float((d != 0).mean()))


@pytest.mark.parametrize("row,R", cases())
def test_radius_build_against_oracle(env, row, R):
    build = rb.BY_NAME[row]
    base = build.options_for(R)
    for label, h, w, extra in shapes(build, R):
        opts = dict(base, **extra)
        try:
            if build.route == "loop":
                run_loop(env, build, R, h, w, opts, TINY_PERSISTENCE if label == "short" else 0.5)
                continue
            for px in build.settings.get("pixel_size", (1,)):
                plan, got, exp = run_api(env, build, R, h, w, opts, px=px)
                assert plan.get("phosphor") == build.plan_for(R) and "blur" not in plan, plan
                assert_bit_exact(got, exp, f"float image, pixel size {px}")
        except AssertionError as e:
            raise AssertionError(f"{row} R={R} {label} {h}x{w} {opts}: {e}") from None


# sigma with 3 sigma on a .5 tie: Python's round() (the reference's, ref:609) goes to the even neighbour
TIES = [(0.5, 2), (1.5, 4), (2.5, 8), (3.5, 10), (7.5, 22), (9.5, 28)]


@pytest.mark.parametrize("sigma,R", TIES)
def test_radius_of_a_rounding_tie(env, sigma, R):
    from pythoncrt_amd import tables
    assert (orc.bloom_ksize(sigma) - 1) // 2 == R and tables.bloom_ksize(sigma) == orc.bloom_ksize(sigma)
    build = rb.BY_NAME["rr_full_u8"]
    plan, got, exp = run_api(env, build, R, 2 * R + 13, 2 * rb.TW + R + 3, build.options_for(R), sigma=sigma)
    assert plan.get("phosphor") == build.plan_for((orc.bloom_ksize(sigma) - 1) // 2), plan
    assert_bit_exact(got, exp, f"sigma {sigma}")


# ---- the split path ---------------------------------------------------------------------------------------------------------------
# It changes shape where sb_steps(R) = (2R + SB_N + 7) & ~7 rounds up (R = 4j -> 4j + 1), where the row pass needs a second LDS chunk
# (sb_steps > SB_CH = 264: R 128 -> 129) and where k_sb_cols_lds's chunk count ceil((24 + sb_steps) / SBC_ROWS) steps (SBC_ROWS = 32:
# R = 16k -> 16k + 1, the radii at which 32 + 2R is a multiple of SBC_ROWS).
SB_N, SB_CH, SBC_ROWS = 8, 264, 32


def sb_steps(R):
    return (2 * R + SB_N + 7) & ~7


SPLIT_RADII = (31, 32, 33, 48, 49, 64, 65, 80, 81, 127, 128, 129, 130, 255, 256, 257)


def test_split_radii_cover_every_boundary():
    """The radii above straddle the first sb_steps round-up of the split path, the row pass's one-chunk limit and the column pass's first
    chunk-count steps (CPU arithmetic on the constants of crtfx_blur.hip.h, restated here)."""
    chunks = lambda R: math.ceil((24 + sb_steps(R)) / SBC_ROWS)      # noqa: E731
    assert sb_steps(32) < sb_steps(33) and sb_steps(64) < sb_steps(65)
    assert sb_steps(128) <= SB_CH < sb_steps(129)
    steps = [R for R in range(31, 257) if chunks(R + 1) > chunks(R)]
    assert steps[:4] == [32, 48, 64, 80] and 128 in steps and 256 in steps, steps
    assert all(R in SPLIT_RADII and R + 1 in SPLIT_RADII for R in steps if R <= 80 or R in (128, 256)), steps


@pytest.mark.parametrize("half", [False, True], ids=["u8", "half"])
@pytest.mark.parametrize("w", [132, 130], ids=["w4", "w2"])
@pytest.mark.parametrize("R", SPLIT_RADII)
def test_split_path_radius_boundaries(env, R, w, half):
    build = rb.Build("split", "", "", "half" if half else "u8", (R,), "api")
    plan, got, exp = run_api(env, build, R, 75, w, {})
    pix = "half" if half else "u8"
    want = f"k_sb_rows<{pix}>+" + ("k_sb_cols_lds" if w % 4 == 0 else "k_sb_cols<1>")
    assert plan.get("blur") == want and "phosphor" not in plan, plan
    assert_bit_exact(got, exp, f"split R={R} {w} {pix}")
