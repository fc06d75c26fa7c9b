"""Every pointwise-chain kernel build held to the oracle, bit for bit.

tests/point_builds.ROWS names every k_point* / k_half* instance the launcher can reach and how it is reached; each row runs on every shape
of point_builds.SHAPES it is reachable on — tiny (2 x 2: smaller than a tile both ways), ragged (34 x 66: a last column strip of 2 pixels, a
last block row of 2 rows, the 34-column half-resolution tile across the strip boundary), strips (50 x 198: four strips, three block rows
plus 2) and, off the fused kernel, odd (37 x 131: the bilinear taps of the half-resolution source instead of the exact 2x decimation).
crtfx_last_plan must name exactly the row's build BEFORE anything is compared, so a planner fallback fails there.

The expected frames are tests/warp_model.render's with the warp off: the oracle's own chain, the image and the persistence state stored
as float32 (tests/test_point_model.py ties that to the unmodified oracle on the CPU).  The kernels draw their own grain; the planes they
drew are exported for the model (crtfx_noise_plane, held to a host model by tests/test_grain_gpu.py; coarse grain: on the small engine),
and so is the 2-D scanline mask of the +scan2d builds (crtfx_scanline_plane, held to the oracle's by tests/test_parity_gpu.py).  Frames,
carried-in states and everything else are drawn on the host.  Bars: np.array_equal everywhere — the uint8 / half frames, every per-frame
float32 state (run one: local_states), the final state, and again with the state kept in registers across the run (run two) — except the
gamma cases (one per grade family, `strips` only): numpy's powf is not the device's, so they keep the suite's gamma bars (state within
3e-7, uint8 <= 1 LSB on < 1e-3 of the samples, half <= 0.125 on < 5e-3).

The last test requires that every instance of the table was named by a plan string some executed case asserted."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import crt_oracle as orc  # noqa: E402  (checker only)
from tests import point_builds as pb  # noqa: E402
from tests import warp_model as wm  # noqa: E402

FPS, FIRST, N = 25.0, 5, 4
SEED = (0x9E3779B9 << 32) | 0x0001E240            # a non-zero high half
PERSISTENCE = {"tiny": 0.2, "ragged": 0.5, "strips": 0.9, "odd": 0.2}
SEEN = set()                                       # instances named by a plan string an executed case asserted
RAN = set()                                        # rows with at least one executed case
PASSED = {}                                        # one passing comparison's (got, expected), for the sensitivity test


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    import pythoncrt_amd
    from pythoncrt_amd import effects
    saved = effects.DEBUG_OPTIONS
    yield pythoncrt_amd, effects, {"opts": None}
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


def device():
    return torch.device("cuda", torch.cuda.current_device())


def describe(got, exp, what):
    """None when equal; else a line that says how many samples differ, by how much and where first."""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.shape != exp.shape or got.dtype != exp.dtype:
        return f"{what}: {got.dtype}{got.shape} against {exp.dtype}{exp.shape}"
    if np.array_equal(got, exp):
        return None
    bad = np.argwhere(got != exp)
    d = np.abs(got.astype(np.float64) - exp.astype(np.float64))
    return f"{what}: {len(bad)} of {got.size} differ; max |d| = {d.max():.3e}; first at {bad[0].tolist()} (got {got[tuple(bad[0])]!r}, model {exp[tuple(bad[0])]!r})"


def require_equal(pairs):
    """pairs: (got, expected, what).  Raises with every mismatch line."""
    bad = [b for b in (describe(g, e, what) for g, e, what in pairs) if b]
    assert not bad, "\n".join(bad[:12])


_CLIPS = {}


def clip(h, w, half):
    """Four frames, drawn once per shape and format: noise; a gradient in both axes; a saturated half with some zero rows; structure + noise.
    Half frames carry fractional values on the 0..255 scale."""
    key = (h, w, half)
    if key not in _CLIPS:
        rng = np.random.default_rng(1000 * h + w + (7 if half else 0))
        yy, xx = np.mgrid[0:h, 0:w]
        grad = np.stack([(xx * 255.0) / max(1, w - 1), (yy * 255.0) / max(1, h - 1), ((xx + yy) * 255.0) / max(1, h + w - 2)], axis=2)
        if half:
            f0 = rng.random((h, w, 3), dtype=np.float32) * 255.0
            f1 = grad.astype(np.float32)
            f2 = rng.random((h, w, 3), dtype=np.float32) * 255.0
            f2[:, : max(1, w // 2)] = 255.0
            f2[::5, w // 2:] = 0.0
            frames = [f.astype(np.float16) for f in (f0, f1, f2)] + [wm.make_frame(h, w, 31, True)]
        else:
            f0 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            f1 = grad.astype(np.uint8)
            f2 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            f2[:, : max(1, w // 2)] = 255
            f2[::5, w // 2:] = 0
            frames = [f0, f1, f2, wm.make_frame(h, w, 31)]
        for f in frames:
            f.setflags(write=False)
        _CLIPS[key] = frames
    return _CLIPS[key]


def export_planes(pipe_engine, cfg, h, w, n, first=FIRST):
    """The grain planes the kernels draw for frames first .. first + n - 1 (coarse grain: drawn at the small size, on an engine of that size)."""
    if cfg["noise_strength"] <= 0.0:
        return None
    from pythoncrt_amd.effects import Engine
    g = cfg["grain_size"]
    gh, gw = (h, w) if g <= 1 else (max(1, h // g), max(1, w // g))
    dev = device()
    eng = pipe_engine if (gh, gw) == (h, w) else Engine(dev, gh, gw, 0)
    planes = []
    for j in range(n):
        p = torch.empty((gh, gw), dtype=torch.float32, device=dev)
        assert eng.lib.crtfx_noise_plane(eng.ctx, SEED, first + j, p.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        planes.append(p.cpu().numpy())
    return planes


def export_scan_planes(eng, cfg, h, w, n):
    """The 2-D scanline masks FramePipeline.frame_records generates for the frames (None: row scanlines or none)."""
    if cfg["scanline_strength"] <= 0.0 or (cfg["scanline_angle"] == 0.0 and cfg["scanline_thickness"] == 1.0):
        return None
    from pythoncrt_amd import tables
    omega, tan_t, inv_sharp = tables.scanline_plane_scalars(cfg["scanline_period_px"], cfg["scanline_angle"], cfg["scanline_thickness"])
    phases = np.arange(FIRST, FIRST + n, dtype=np.int64).astype(np.float64) / FPS * cfg["scanline_speed_px_s"]
    dev = device()
    out = []
    for ph in phases:
        p = torch.empty((h, w), dtype=torch.float32, device=dev)
        assert eng.lib.crtfx_scanline_plane(eng.ctx, float(cfg["scanline_strength"]), omega, float(ph), tan_t, inv_sharp, p.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream) == 0
        out.append(p.cpu().numpy())
    return out


def render_settings(cfg):
    from pythoncrt_amd.pipeline import RenderSettings
    return RenderSettings(**cfg)


def assert_plan(plan, row, h, w, frames, float_out=False, group_min=None):
    """crtfx_last_plan names exactly the row's build (and the restated launcher agrees on this very shape); notes the instances it names."""
    want = pb.default_point_plan(row.settings, row.pix, h, w, row.options, row.blend, frames, float_out)
    assert want["point"] == row.point and want.get("half", "") == row.half, (row.name, want)
    assert plan.get("point") == row.point, f"{row.name}: plan {plan}, expected point={row.point}"
    assert plan.get("half", "") == row.half, f"{row.name}: plan {plan}, expected half={row.half!r}"
    if group_min is not None:
        assert int(plan.get("group", 0)) >= group_min, f"{row.name}: plan {plan}: the asserted launch took fewer than {group_min} frames"
    SEEN.add(pb.plan_instance(plan["point"]))
    if plan.get("half"):
        SEEN.add(pb.plan_instance(plan["half"]))


def run_pipeline(env, row, cfg, h, w, n, state0, local):
    """n frames through FramePipeline.run -> (plan, frames, final state or None, per-frame states or None, the exported planes)."""
    from pythoncrt_amd.pipeline import FramePipeline
    use_options(env, row.options)
    half = row.pix == "half"
    dev = device()
    pipe = FramePipeline(dev, h, w, render_settings(cfg), fps=FPS, noise_seed=SEED, dtype=torch.float16 if half else torch.uint8)
    frames = torch.from_numpy(np.stack(clip(h, w, half)[:n])).to(dev)
    keep = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev) if local else None
    st_in = torch.from_numpy(state0.copy()).to(dev) if state0 is not None else None
    out, st = pipe.run(frames, first_index=FIRST, state=st_in, local_states=keep)
    plan = pipe.plan()
    res = (plan, out.cpu().numpy(), st.cpu().numpy() if st is not None else None, keep.cpu().numpy() if keep is not None else None)
    planes = export_planes(pipe.engine, cfg, h, w, n), export_scan_planes(pipe.engine, cfg, h, w, n)
    return res + planes


def loop_case(env, row, shape, gamma=None):
    """-> (model frames, model states, run one, run two or None): the compared pieces of one loop / single case."""
    h, w = pb.SHAPES[shape]
    half = row.pix == "half"
    single = row.route == "single"
    n = 1 if single else N
    p = PERSISTENCE[shape] if row.blend == "render" else 0.0
    cfg = dict(pb.DEFAULTS, **row.settings, persistence=p)
    if gamma is not None:
        cfg["gamma"] = gamma
    state0 = wm.make_state(h, w, 7 * h + w) if row.blend == "render" else None
    plan, out, st, keep, planes, scan = run_pipeline(env, row, cfg, h, w, n, state0, local=row.blend == "render")
    # the plan first: a planner fallback fails here and never passes against another kernel
    assert_plan(plan, row, h, w, n, group_min=None if single else 2)
    assert int(plan.get("group", 0)) == (1 if single else n), plan
    m_out, m_states = wm.point_render(clip(h, w, half)[:n], cfg, half, FPS, FIRST, planes, state0, scan)
    two = None
    if row.blend == "render":
        plan2, out2, st2, _, _, _ = run_pipeline(env, row, cfg, h, w, n, state0, local=False)      # the state stays in registers across the run
        assert_plan(plan2, row, h, w, n, group_min=None if single else 2)
        two = (out2, st2)
    return cfg, m_out, m_states, (out, st, keep), two


CASES = [(r.name, k) for r in sorted(pb.ROWS, key=lambda r: sorted(r.options.items())) for k in pb.row_shapes(r)]


@pytest.mark.parametrize("name,shape", CASES, ids=[f"{n}-{k}" for n, k in CASES])
def test_point_build_against_oracle(env, name, shape):
    row = pb.BY_NAME[name]
    RAN.add(name)
    try:
        if row.route == "api":
            return api_case(env, row, shape)
        cfg, m_out, m_states, (out, st, keep), two = loop_case(env, row, shape)
    except (RuntimeError, OSError) as e:          # a HIP error (CrtfxError is a RuntimeError): nothing more is started on a device that reported one
        pytest.exit(f"{name}-{shape}: {type(e).__name__}: {e}", returncode=3)
    n = len(m_out)
    pairs = [(out[j], m_out[j], f"frame {j}") for j in range(n)]
    if row.blend == "render":
        pairs += [(keep[j], m_states[j], f"per-frame state {j}") for j in range(n)]
        pairs += [(wm.quantise(keep[j], row.pix == "half"), out[j], f"frame {j} against its own state, quantised") for j in range(n)]
        pairs.append((st, m_states[-1], "final state"))
        pairs += [(two[0][j], m_out[j], f"state in registers: frame {j}") for j in range(n)]
        pairs.append((two[1], m_states[-1], "state in registers: final state"))
    else:
        assert st is None
    require_equal(pairs)
    PASSED["pair"] = (out[0].copy(), m_out[0].copy())
    if row.route == "single" and row.blend == "none":
        # one frame at the start of a persistence chain: it passes through unblended and leaves its float32 state behind
        cfg2 = dict(cfg, persistence=0.5)
        plan, out, st, _, planes, scan = run_pipeline(env, row, cfg2, *pb.SHAPES[shape], 1, None, local=False)
        assert_plan(plan, row, *pb.SHAPES[shape], 1)
        require_equal([(out[0], m_out[0], "chain start: frame"), (st, m_states[0], "chain start: state")])


def api_case(env, row, shape):
    """apply_static_effects' float image against float32(the oracle's image)."""
    pc, effects, _ = env
    from pythoncrt_amd import _lib
    use_options(env, row.options)
    h, w = pb.SHAPES[shape]
    half = row.pix == "half"
    cfg = dict(pb.DEFAULTS, **row.settings)
    frame = clip(h, w, half)[3 if shape == "tiny" else 2]
    phase, t_sec = 1.25, FIRST / FPS
    kw = {k: cfg[k] for k in wm.POINT_KEYS}

    def args(mod):
        tm = mod.make_triad_mask(h, w, cfg["triad_strength"], cfg["triad_softness"]) if cfg["triad_strength"] > 0.0 else None
        vg = mod.make_vignette(h, w, cfg["vignette_strength"]) if cfg["vignette_strength"] > 0.0 else None
        return (frame, cfg["scanline_strength"], tm, cfg["triad_gamma"], cfg["triad_preserve_luma"], cfg["aberration_px"], cfg["bloom_sigma"],
                cfg["bloom_strength"], cfg["bloom_threshold"], cfg["noise_strength"], vg, cfg["scanline_period_px"], phase, cfg["fast_bloom"],
                cfg["pixel_size"], 0, 0.0)
    got = pc.apply_static_effects(*args(pc), time_sec=t_sec, noise_seed=SEED, frame_index=FIRST, **kw)
    eng = effects._engine(device(), h, w, _lib.PIX_F16 if half else _lib.PIX_U8)
    assert_plan(eng.last_plan(), row, h, w, 1, float_out=True)
    planes = export_planes(eng, cfg, h, w, 1)
    exp = orc.apply_static_effects(*args(orc), time_sec=t_sec, noise_plane=None if planes is None else planes[0], **kw)
    assert exp.dtype == (np.float64 if wm.promoted(cfg) else np.float32)
    require_equal([(got, exp.astype(np.float32), "float image")])


GAMMA_ROWS = [r.name for r in pb.ROWS if r.gamma_family]


@pytest.mark.parametrize("name", GAMMA_ROWS)
def test_gamma_case_of_every_grade_family(env, name):
    """gamma != 1: the oracle's np.power and the device's powf differ in the last place, so these keep the suite's gamma bars — float state
    within 3e-7 of the model, uint8 <= 1 LSB on < 1e-3 of the samples, half <= 0.125 on < 5e-3 — on `strips` only (a rate needs the samples)."""
    row = pb.BY_NAME[name]
    half = row.pix == "half"
    _, m_out, m_states, (out, st, keep), two = loop_case(env, row, "strips", gamma=1.8)
    for frames, what in ((out, "run one"), (two[0], "state in registers")):
        for j in range(N):
            d = np.abs(frames[j].astype(np.float32) - m_out[j].astype(np.float32))
            rate = float((frames[j] != m_out[j]).mean())
            print(f"{name} {what} frame {j}: max |d| = {float(d.max())}, rate = {rate:.2e}")
            assert d.max() <= (0.125 if half else 1) and rate < (5e-3 if half else 1e-3), (name, what, j, float(d.max()), rate)
    for j in range(N):
        ds = float(np.abs(keep[j].astype(np.float64) - m_states[j]).max())
        print(f"{name} state {j}: max |d| = {ds:.3e}")
        assert ds <= 3e-7, (name, j, ds)
    assert float(np.abs(st.astype(np.float64) - m_states[-1]).max()) <= 3e-7 and float(np.abs(two[1].astype(np.float64) - m_states[-1]).max()) <= 3e-7


def test_one_flipped_sample_fails_the_comparison():
    """The comparison helper raises on ONE sample one LSB off (a host copy of a passing case's frame; the kernels are not touched)."""
    if "pair" in PASSED:
        got, exp = PASSED["pair"]
    else:
        exp = wm.make_frame(6, 9, 3)
        got = exp.copy()
    require_equal([(got, exp, "untouched")])
    for idx in ((0, 0, 0), tuple(s - 1 for s in got.shape)):
        bad = got.copy()
        if bad.dtype == np.uint8:
            bad[idx] = bad[idx] + 1 if bad[idx] < 255 else 254
        else:
            bad[idx] = np.nextafter(bad[idx], np.float16(np.inf))          # one half ulp up
        assert describe(bad, exp, "flipped") is not None
        with pytest.raises(AssertionError, match="1 of"):
            require_equal([(got, exp, "untouched"), (bad, exp, "flipped")])
    st = wm.make_state(4, 5, 1)
    bad = st.copy()
    bad[3, 4, 2] = np.nextafter(bad[3, 4, 2], np.float32(2.0))            # one float32 ulp in a state
    with pytest.raises(AssertionError, match="1 of"):
        require_equal([(bad, st, "state")])


def test_every_instance_was_asserted_by_an_executed_case():
    """Every k_point* / k_half* instance of the table (= of the library: tests/test_evidence_tools.py) was named by a plan string that an
    executed case asserted.  With a selection of the cases (-k) only the selected rows' instances are required."""
    required = {k for r in pb.ROWS if r.name in RAN for k in r.kernels}
    missing = sorted(required - SEEN)
    print(f"instances asserted: {len(SEEN)}; required: {len(required)}; never asserted: {missing}")
    assert not missing, missing
    if len(RAN) == len(pb.ROWS):
        assert SEEN == pb.covered_instances() and len(SEEN) == 115, sorted(pb.covered_instances() ^ SEEN)
