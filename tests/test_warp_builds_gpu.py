"""Every warp / commit kernel build held to the float32-storage model, bit for bit.

The warp used to be the one stage compared to the oracle by tolerance (3e-7 / 1 LSB on < 0.1 % / one half ulp on < 0.5 % / 4e-7): the oracle
interpolates the reference's float64 image, the GPU the image it stored as float32.  tests/warp_model.py composes the oracle's own functions
with exactly those float32 roundings (tests/test_warp_model.py ties it to the unmodified oracle at the old bars, on the CPU), and everything
else the kernels do is deterministic arithmetic — so here the uint8 / half frames, every returned or parked persistence state and the float
image of the `api` route must EQUAL the model (np.array_equal, no sample allowance), and no GPU output feeds the model: frames, injected
grain planes and carried-in states are all drawn on the host.

tests/warp_builds.ROWS names every reachable instance and how it is reached; each row runs every strength of warp_model.STRENGTHS on every
shape of warp_model.SHAPES its width condition admits (the shapes span W % 4 in {0, 1, 2, 3}; W below, at and one past a 64- / 128-pixel
tile; H below the rows one thread owns; H % 8, 16, 32 != 0), and crtfx_last_plan must name exactly the row's build in every case.  Along the
cases of a row the run parameters rotate: 1, 2, 5 and 8 frames; persistence 0.2, 0.5, 0.97; a chain started from a supplied state or from
none; launch groups of the planner's size, 3 and 8 (so 5 and 8 frames span several launches); the unpromoted chain (all gates off) and the
promoted ones (scanlines + vignette, grouped into multi-frame launches; the full gate set with an injected grain plane, one frame per
launch).  A second sweep runs the planner's default build of every route on every shape.

The 2^31-byte boundary of the lean kernel's buffer resource (test_buffer_resource_boundary): 5462 x 32764 (H * W * 12 = 2^31 - 32, W % 4 =
0: the plain build), its transpose (W % 4 = 2: the general lean build) and 32764 x 5463, one column past the boundary (the general k_warp).
Its wall time is recorded in that test's docstring."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import crt_oracle as orc  # noqa: E402  (checker only)
from tests import warp_builds as wb  # noqa: E402
from tests import warp_model as wm  # noqa: E402

FIRST = 3                                   # frame index of the first frame (scanline phase)
FRAMES = (1, 2, 5, 8)
PERSISTENCE = (0.2, 0.5, 0.97)
GROUPS = (0, 3, 8)                          # CRTFX_OPT_GROUP: the planner's choice, 3, 8
BANDED_SHAPES = ((520, 448), (300, 704), (416, 512), (301, 449), (290, 450))      # pre-warp images of more than 1 MiB: BAND_MB = 1 cuts them into bands


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    import pythoncrt_amd
    from pythoncrt_amd import effects
    saved = effects.DEBUG_OPTIONS
    yield pythoncrt_amd, effects
    effects.DEBUG_OPTIONS = saved
    effects._tls.engines = {}
    torch.cuda.empty_cache()


def device():
    return torch.device("cuda", torch.cuda.current_device())


def describe(got, exp, what):
    """None when equal; else a line that says how many samples differ, by how much and where first."""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.shape == exp.shape and got.dtype == exp.dtype and np.array_equal(got, exp):
        return None
    if got.shape != exp.shape or got.dtype != exp.dtype:
        return f"{what}: {got.dtype}{got.shape} against {exp.dtype}{exp.shape}"
    bad = np.argwhere(got != exp)
    d = np.abs(got.astype(np.float64) - exp.astype(np.float64))
    return f"{what}: {len(bad)} of {got.size} differ; max |d| = {d.max():.3e}; first at {bad[0].tolist()} (got {got[tuple(bad[0])]!r}, model {exp[tuple(bad[0])]!r})"


def chain_cfg(row, k):
    """The effect settings of case k of a row: the chain dtype the row names, on a gate set its route can take."""
    if row.route == "commit" or row.extra.get("banded"):
        return wm.BLOOM64 if row.chain == "f64" else wm.BLOOM32      # the Gaussian chain (bands and the commit-only build sit behind it)
    if row.chain == "f32":
        return wm.OFF
    return wm.FULL if k % 3 == 0 else wm.VIG


def render_settings(cfg):
    from pythoncrt_amd.pipeline import RenderSettings
    return RenderSettings(**{k: v for k, v in cfg.items() if k not in ("glitch_amp_px", "glitch_height_frac")})


def run_loop(env, row, cfg, h, w, n, opts, from_state, per_frame_states, seed):
    """n frames through FramePipeline.run -> (plan, list of mismatch lines)."""
    _, effects = env
    from pythoncrt_amd.pipeline import FramePipeline
    half = row.pix == "half"
    dev = device()
    frames = [wm.make_frame(h, w, seed + j, half) for j in range(n)]
    planes = [wm.make_plane(h, w, seed + 50 + j) for j in range(n)] if cfg["noise_strength"] > 0.0 else None
    state0 = wm.make_state(h, w, seed + 99) if (from_state and cfg["persistence"] > 0.0) else None
    effects.DEBUG_OPTIONS = dict(opts)          # FramePipeline makes its own ctx
    pipe = FramePipeline(dev, h, w, render_settings(cfg), fps=30.0, noise_seed=1, dtype=torch.float16 if half else torch.uint8)
    local = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev) if per_frame_states else None
    st_in = torch.from_numpy(state0.copy()).to(dev) if state0 is not None else None
    out, st = pipe.run(torch.from_numpy(np.stack(frames)).to(dev), first_index=FIRST, state=st_in,
                       noise_planes=torch.from_numpy(np.stack(planes)).to(dev) if planes is not None else None, local_states=local)
    plan = pipe.plan()
    out = out.cpu().numpy()
    st = st.cpu().numpy() if st is not None else None
    local = local.cpu().numpy() if local is not None else None
    del pipe
    m_out, m_states = wm.render(frames, cfg, half, first=FIRST, planes=planes, state=state0)
    bad = [describe(out[j], m_out[j], f"frame {j}") for j in range(n)]
    if cfg["persistence"] > 0.0:
        bad.append(describe(st, m_states[-1], "carried state"))
    if local is not None:
        bad += [describe(local[j], m_states[j], f"local state {j}") for j in range(n)]
    return plan, [b for b in bad if b]


def api_args(frame, cfg, tm, vg, phase, glitch):
    return (frame, cfg["scanline_strength"], tm, cfg["triad_gamma"], cfg["triad_preserve_luma"], cfg["aberration_px"], cfg["bloom_sigma"],
            cfg["bloom_strength"], cfg["bloom_threshold"], cfg["noise_strength"], vg, cfg["scanline_period_px"], phase, cfg["fast_bloom"],
            cfg["pixel_size"], glitch[0], glitch[1])


def masks(mod, cfg, h, w):
    tm = mod.make_triad_mask(h, w, cfg["triad_strength"], cfg["triad_softness"]) if cfg["triad_strength"] > 0.0 else None
    vg = mod.make_vignette(h, w, cfg["vignette_strength"]) if cfg["vignette_strength"] > 0.0 else None
    return tm, vg


def pre_image(frame, cfg, h, w, phase, plane):
    """The pre-warp image of the api / preview routes as the GPU holds it (warp_model.pre_images restated for those entry points)."""
    pre = orc.apply_static_effects(*api_args(frame, cfg, *masks(orc, cfg, h, w), phase, (0, 0.0)), noise_plane=plane, stop_before_warp=True)
    assert pre.dtype == (np.float64 if wm.promoted(cfg) else np.float32)
    return pre.astype(np.float32).astype(pre.dtype)


def run_api(env, row, cfg, h, w, s, seed):
    pc, effects = env
    if effects.DEBUG_OPTIONS != row.options:
        effects.DEBUG_OPTIONS = dict(row.options)
        effects._tls.engines = {}
    from pythoncrt_amd import _lib
    half = row.pix == "half"
    frame = wm.make_frame(h, w, seed, half)
    plane = wm.make_plane(h, w, seed + 50) if cfg["noise_strength"] > 0.0 else None
    phase = 1.25
    glitch = (6, 0.25) if row.extra.get("glitch") else (0, 0.0)
    got = pc.apply_static_effects(*api_args(frame, cfg, *masks(pc, cfg, h, w), phase, glitch), warp_strength=s, noise_plane=plane)
    plan = effects._engine(device(), h, w, _lib.PIX_F16 if half else _lib.PIX_U8).last_plan()
    g = orc.glitch_offsets_render(h, w, phase, *glitch) if glitch[0] else None
    exp = wm.static_image(pre_image(frame, cfg, h, w, phase, plane), s, g)
    bad = describe(got, exp, "float image")
    return plan, [bad] if bad else []


def run_preview(env, row, cfg, h, w, s, n, p, seed):
    """n apply_crt_effect ticks threaded through state_prev; the plan is the last tick's."""
    pc, effects = env
    if effects.DEBUG_OPTIONS != row.options:
        effects.DEBUG_OPTIONS = dict(row.options)
        effects._tls.engines = {}
    glitch = (6, 0.25) if row.extra.get("glitch") else (0, 0.0)
    sg = sm = None
    bad = []
    for i in range(n):
        frame = wm.make_frame(h, w, seed + i)
        plane = wm.make_plane(h, w, seed + 50 + i) if cfg["noise_strength"] > 0.0 else None
        phase = float(i)
        a = api_args(frame, cfg, *masks(pc, cfg, h, w), phase, (0, 0.0))
        ug, sg = pc.apply_crt_effect(*(a[:11] + (p, sg) + a[11:15]), glitch[0], glitch[1], warp_strength=s, noise_plane=plane)
        g = orc.glitch_offsets_preview(h, w, phase, *glitch) if glitch[0] else None
        um, sm = wm.preview_step(wm.warp(pre_image(frame, cfg, h, w, phase, plane), s, g), p, sm)
        bad += [describe(ug, um, f"tick {i} frame"), describe(np.asarray(sg), sm, f"tick {i} state")]
    plan = effects._engine(device(), h, w).last_plan()
    return plan, [b for b in bad if b]


def row_shapes(row):
    if row.extra.get("banded"):
        return [s for s in BANDED_SHAPES if row.fits(s[1])]
    shapes = [s for s in wm.SHAPES if row.fits(s[1])]
    if row.extra.get("glitch"):
        shapes = [s for s in shapes if s[0] >= 8]          # a band of at least two rows
    return shapes


def test_every_row_gets_the_residue_classes():
    """Every row runs on at least three shapes; the rows open to any width see W % 4 in {0, 1, 2, 3}, a width one past a 128-pixel tile
    and a height below the rows one thread owns; the half rows see W odd, W % 4 = 2 and W % 4 = 0 (CPU arithmetic on the tables)."""
    for row in wb.ROWS:
        shapes = row_shapes(row)
        assert len(shapes) >= 3, row.name
        res = {w % 4 for _, w in shapes}
        if row.extra.get("banded"):
            assert res >= ({0} if row.widths == "w4" else {0, 1, 2}), row.name
            continue
        want = {"any": {0, 1, 2, 3}, "w2": {0, 2}, "w4": {0}}[row.widths]
        assert res >= want, (row.name, res)
        if row.widths == "any" and not row.extra.get("glitch"):
            assert any(w == 129 for _, w in shapes) and any(h < 4 for h, _ in shapes), row.name
        assert any(h % 8 and h % 16 and h % 32 for h, _ in shapes), row.name


@pytest.mark.parametrize("name", [r.name for r in wb.ROWS])
def test_warp_build_against_model(env, name):
    row = wb.BY_NAME[name]
    shapes = row_shapes(row)
    strengths = (0.0,) if (row.route == "commit" or row.extra.get("no_warp")) else wm.STRENGTHS
    failures, multi = [], 0
    seen_general_multi = False
    k = 0
    for s in strengths:
        for h, w in shapes:
            k += 1
            cfg = dict(chain_cfg(row, k), warp_strength=s)
            n = FRAMES[k % 4]
            p = PERSISTENCE[k % 3] if row.blend in ("render", "preview") else 0.0
            seed = 1000 * k + 17
            if row.route in ("loop", "commit"):
                opts = dict(row.options)
                opts.setdefault("GROUP", GROUPS[(k // 4) % 3])
                if row.extra.get("banded"):
                    n = 2
                # a chain started from none commits its first frame unblended (another build): one frame alone needs a state to blend with
                from_state = (k // 2) % 2 == 1 or (n == 1 and row.blend == "render")
                plan, bad = run_loop(env, row, dict(cfg, persistence=p), h, w, n, opts, from_state, bool(row.extra.get("local_states")), seed)
                multi = max(multi, int(plan.get("warp_frames", 0)))
            elif row.route == "api":
                plan, bad = run_api(env, row, cfg, h, w, s, seed)
            else:
                plan, bad = run_preview(env, row, cfg, h, w, s, max(2, n if n < 8 else 4), p, seed)
            want = row.plan
            if row.extra.get("local_states") and int(plan.get("warp_frames", 0)) < 2:
                # a launch of ONE frame names one state buffer, so on rows of whole dwords the launcher may take the branch-free build;
                # the launches of several frames (each frame its own buffer) must take the general one
                want = wb.default_plan(row.chain, row.blend, row.pix, h, w, opts)
            elif row.extra.get("local_states"):
                seen_general_multi = True
            if plan.get("warp") != want:
                bad.insert(0, f"plan {plan}, expected {want}")
            if bad:
                failures.append(f"{h}x{w} s={s} n={n} p={p} cfg={'/'.join(k_ for k_, v in cfg.items() if v and k_ in ('bloom_strength', 'vignette_strength', 'noise_strength', 'scanline_strength'))}: " + "; ".join(bad[:4]))
    assert not failures, f"{row.name} ({row.plan}): {len(failures)} of {k} cases fail:\n" + "\n".join(failures[:25])
    if row.kernel.startswith("crtfx::k_warp_lean<") and not row.extra.get("banded"):
        assert multi >= 2, f"{row.name}: no launch of this row took more than one frame"
    if row.extra.get("local_states"):
        assert seen_general_multi, f"{row.name}: no multi-frame launch with per-frame state buffers"


DEFAULT_ROUTES = [(chain, blend, pix) for chain in ("f32", "f64") for blend in ("none", "render") for pix in ("u8", "half")]


@pytest.mark.parametrize("chain,blend,pix", DEFAULT_ROUTES)
def test_default_build_on_every_shape(env, chain, blend, pix):
    """The planner's own choice (no DEBUG_OPTIONS) of the render loop on every shape, both chains, both blends, both pixel formats."""
    failures = []
    for k, (h, w) in enumerate(wm.SHAPES):
        s = wm.STRENGTHS[k % len(wm.STRENGTHS)]
        row = wb.Row("default", "", "loop", chain, blend, pix)
        cfg = dict(chain_cfg(row, k), warp_strength=s, persistence=PERSISTENCE[k % 3] if blend == "render" else 0.0)
        n = FRAMES[1 + k % 3]
        plan, bad = run_loop(env, row, cfg, h, w, n, {}, k % 2 == 1, False, 500 * k + 3)
        want = wb.default_plan(chain, blend, pix, h, w)
        if plan.get("warp") != want:
            bad.insert(0, f"plan {plan}, expected {want}")
        if bad:
            failures.append(f"{h}x{w} s={s} n={n}: " + "; ".join(bad[:4]))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("chain", ["f32", "f64"])
def test_default_build_of_the_api_and_preview_routes_on_every_shape(env, chain):
    failures = []
    for k, (h, w) in enumerate(wm.SHAPES):
        s = wm.STRENGTHS[(k + 3) % len(wm.STRENGTHS)]
        cfg = dict(wm.OFF if chain == "f32" else (wm.FULL if k % 2 else wm.VIG), warp_strength=s)
        for row in (wb.BY_NAME[f"general_{chain}_api_u8"], wb.BY_NAME[f"general_{chain}_preview"]):
            if row.route == "api":
                plan, bad = run_api(env, row, cfg, h, w, s, 300 * k + 1)
            else:
                plan, bad = run_preview(env, row, cfg, h, w, s, 3, 0.5, 300 * k + 2)
            if plan.get("warp") != row.plan:
                bad.insert(0, f"plan {plan}")
            if bad:
                failures.append(f"{row.name} {h}x{w} s={s}: " + "; ".join(bad[:4]))
    # the first preview tick has no state to blend with: an unblended lean launch that also stores its float state
    pc, effects = env
    h, w = 37, 129
    frame = wm.make_frame(h, w, 77)
    cfg = dict(wm.OFF if chain == "f32" else wm.VIG, warp_strength=0.15)
    a = api_args(frame, cfg, *masks(pc, cfg, h, w), 2.0, (0, 0.0))
    ug, sg = pc.apply_crt_effect(*(a[:11] + (0.5, None) + a[11:15]), warp_strength=0.15)
    plan = effects._engine(device(), h, w).last_plan()
    um, sm = wm.preview_step(wm.warp(pre_image(frame, cfg, h, w, 2.0, None), 0.15), 0.5, None)
    if plan.get("warp") != wb.default_plan(chain, "none", "u8", h, w, keeps_state=True):
        failures.append(f"first tick: plan {plan}")
    failures += [b for b in (describe(ug, um, "first tick frame"), describe(np.asarray(sg), sm, "first tick state")) if b]
    assert not failures, "\n".join(failures)


BOUNDARY = [(5462, 32764, "k_warp_lean<f32,none,u8,rows=4,tile=128x8,plain>"),
            (32764, 5462, "k_warp_lean<f32,none,u8,rows=4,tile=128x8,general>"),
            (32764, 5463, "k_warp<gather>")]


@pytest.mark.parametrize("h,w,want", BOUNDARY)
def test_buffer_resource_boundary(env, h, w, want):
    """The largest offsets k_warp_lean's __mul24 / 32-bit offset arithmetic ever sees: H * W * 12 = 2^31 - 32 bytes (both orientations), and
    one column past 2^31, where the launcher must route to the general k_warp.  Unpromoted chain, strength 0.15, one frame.
    Wall time measured on an MI355X host: 5.1 s (5462 x 32764), 6.1 s (32764 x 5462), 6.2 s (32764 x 5463) per case, nearly all of it the host
    model's remap of 179 M pixels (about 7.5 GB of host memory at its peak)."""
    _, effects = env
    assert h * w * 12 == (1 << 31) - 32 or h * w * 12 > 1 << 31
    assert wb.default_plan("f32", "none", "u8", h, w) == want
    from pythoncrt_amd.pipeline import FramePipeline
    cfg = dict(wm.OFF, warp_strength=0.15)
    rng = np.random.default_rng(h)
    frame = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    effects.DEBUG_OPTIONS = {}
    dev = device()
    pipe = FramePipeline(dev, h, w, render_settings(cfg), fps=30.0, noise_seed=1)
    out, _ = pipe.run(torch.from_numpy(frame[None]).to(dev), first_index=0)
    plan = pipe.plan()
    out = out.cpu().numpy()[0]
    del pipe
    torch.cuda.empty_cache()
    assert plan.get("warp") == want, plan
    m_out, _ = wm.render([frame], cfg)
    bad = describe(out, m_out[0], "frame")
    assert bad is None, bad
    assert out[h // 2, w // 2].any() and not out[0, 0].any()      # the centre is lit, the barrel's corner samples outside
