"""A ctx reused across parameter changes against a ctx created for each parameter set.

Every other GPU test runs its kernels on a ctx that was created (or whose engine cache was cleared) just before the case it checks; the
product keeps one ctx per (device, size, format, thread) and calls crtfx_set_params again whenever a keyword changes.  Here ONE ctx lives
for a whole walk of tests/ctx_transitions.py (star: base -> X -> base for every stop; pairs: every arrow both ways; random: 40 seeded
steps), on both routes (`api`: apply_static_effects + apply_crt_effect on the drop-in's cached Engine; `loop`: FramePipeline.set_settings
+ run), both pixel formats and the two sizes.  After every step:

  * reused equals fresh, bit for bit: frames, the float image, the persistence state, per-frame local states (loop, and again with the
    state kept in registers) against the same call on a ctx created for that stop (`effects._tls.engines = {}` / a new FramePipeline),
    computed once per (stop, size, format, route);
  * same plan: crtfx_last_plan of the reused ctx is the fresh ctx's dict, and the fresh plan starts with the stop's family prefix;
  * anchored: each fresh result is held to the oracle once with the bars the suite already uses for the route — api float image bit-exact
    with no warp and no grade gamma, else <= 3e-7; preview state <= 4e-7; loop state <= 1e-6; uint8 frames <= 1 LSB on <= 2e-3 of the
    samples; half frames <= 0.125 on < 5e-3 — with the grain planes the kernels drew exported for it (crtfx_noise_plane).  Where the grade
    gamma is the device's powf (half frames), a sample whose triad-LUT index the oracle itself flips when its own power result moves by
    one ulp passes inside the oracle's envelope instead (float_miss, powf_nudged); every other sample keeps the bar.

tests/test_ctx_transitions.py shows on the CPU that every step changes >= 5 % of the float samples and >= 1 % of the uint8 ones, so a
table, plan field or scratch buffer left over from the previous stop cannot pass.  One more case threads the state through 12 ticks with
another stop on every tick and a frame size change in the middle; four cases hold the Python-side mask caches."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import crt_oracle as orc  # noqa: E402  (checker only)
from tests import ctx_transitions as ct  # noqa: E402

FPS, FIRST, N = 25.0, 3, 6                          # 6 frames from index 3, persistence 0.5: a full in-register run behind the first frame
SEED = (0x9E3779B9 << 32) | 0x0001E240
PERSISTENCE = 0.5
FRESH = {}                                          # (route, stop, size, pix) -> the fresh ctx's results (+ "anchor": None or what missed the oracle's bars)
STEPS_RUN = [0]


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    import pythoncrt_amd
    from pythoncrt_amd import effects
    effects._tls.engines = {}
    yield pythoncrt_amd, effects
    effects._tls.engines = {}
    FRESH.clear()
    torch.cuda.empty_cache()


def device():
    return torch.device("cuda", torch.cuda.current_device())


def pix_fmt(pix):
    from pythoncrt_amd import _lib
    return _lib.PIX_F16 if pix == "half" else _lib.PIX_U8


_INPUTS = {}


def inputs(size, pix):
    """One frame (api), six frames (loop) and the carried-in state of a size and format: drawn once, read-only."""
    key = (size, pix)
    if key not in _INPUTS:
        h, w = ct.SIZES[size]
        half = pix == "half"
        d = dict(frame=ct.make_frame(h, w, 3, half), clip=np.stack([ct.make_frame(h, w, 10 + j, half) for j in range(N)]), state=ct.make_state(h, w, 21),
                 planes=ct.plane_masks(h, w, 5))
        for k in ("frame", "clip", "state"):
            d[k].setflags(write=False)
        _INPUTS[key] = d
    return _INPUTS[key]


def masks(mod, stop, size, pix):
    h, w = ct.SIZES[size]
    return inputs(size, pix)["planes"] if stop.settings.get("_planes") else ct.api_masks(mod, stop, h, w)


def export_planes(eng, cfg, h, w, indices):
    """The grain planes the kernels draw for the frame indices (coarse grain: at the small size, on an engine of that size); None = no grain."""
    if cfg["noise_strength"] <= 0.0:
        return None
    from pythoncrt_amd.effects import Engine
    g = cfg["grain_size"]
    gh, gw = (h, w) if g <= 1 else (max(1, h // g), max(1, w // g))
    small = eng if (gh, gw) == (h, w) else Engine(device(), gh, gw, 0)
    out = []
    for i in indices:
        p = torch.empty((gh, gw), dtype=torch.float32, device=device())
        assert small.lib.crtfx_noise_plane(small.ctx, SEED, i, p.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        out.append(p.cpu().numpy())
    return out


def u8_miss(got, exp, what):
    d = np.abs(got.astype(np.int16) - exp.astype(np.int16))
    rate = float((d != 0).mean())
    return None if d.max() <= 1 and rate <= max(2e-3, 2.0 / d.size) else f"{what}: max {int(d.max())} LSB, {rate:.2e} of the samples off"


def half_miss(got, state64, what):
    exp16 = np.abs(state64.astype(np.float32) * np.float32(255.0)).astype(np.float16)
    d = np.abs(got.astype(np.float32) - exp16.astype(np.float32))
    rate = float((got != exp16).mean())
    return None if d.max() <= 0.125 and rate < 5e-3 else f"{what}: max {float(d.max())}, {rate:.2e} of the half samples off"


def float_miss(got, exp, bar, what, variants=()):
    """`variants`: the oracle's result with its grade gamma one float32 ulp up / down (powf_nudged).  A sample passes within `bar` of the
    oracle; where the oracle's own variants are more than 1e-6 apart — a truncated triad-LUT index that one ulp of powf flips — it passes
    inside their envelope, widened by `bar`.  Every other sample keeps the bar."""
    if bar == 0.0:
        return None if np.array_equal(got, exp.astype(np.float32)) else f"{what}: {int((got != exp.astype(np.float32)).sum())} of {got.size} samples differ from float32(oracle)"
    g = got.astype(np.float64)
    d = np.abs(g - exp)
    if variants:
        lo, hi = np.minimum.reduce([exp, *variants]), np.maximum.reduce([exp, *variants])
        flips = (hi - lo) > 1e-6
        d = np.where(flips & (g >= lo - bar) & (g <= hi + bar), 0.0, d)
    err = float(d.max())
    return None if err <= bar else f"{what}: max |d| = {err:.3e} > {bar} ({int((d > bar).sum())} samples)"


def device_powf(cfg, pix):
    """The grade gamma of this stop is the device's powf (uint8 frames read numpy's own values from the host-built grade table unless a
    saturation stands next to it): numpy's power differs from it in the last place (the suite's gamma bars, 3e-7)."""
    return cfg["gamma"] != 1.0 and cfg["gamma"] > 0.0 and (pix == "half" or cfg["saturation"] != 1.0)


class powf_nudged:
    """The oracle with the result of its grade gamma moved one float32 ulp up (+1) or down (-1): what another correctly rounded-to-an-ulp powf
    may return.  The reference truncates that value to a triad-LUT index right behind it (ref:246-263), so a value that sits on an index edge
    flips to the neighbouring entry (~1e-3) — found here: 0.8818359 = 903 / 1024 exactly, loop route, half frames, gamma 1.3."""

    def __init__(self, direction):
        self.direction = direction

    def __enter__(self):
        self.real = real = orc.apply_color_adjustments
        towards = np.float32(2.0 if self.direction > 0 else -1.0)

        def nudged(img, brightness, contrast, gamma, saturation, temperature):
            out = real(img, brightness, contrast, gamma, saturation, temperature)
            if gamma != 1.0 and gamma > 0.0:
                out = np.clip(np.nextafter(out.astype(np.float32), towards), 0.0, 1.0).astype(np.float32)
            return out
        orc.apply_color_adjustments = nudged

    def __exit__(self, *exc):
        orc.apply_color_adjustments = self.real
        return False


def oracle_variants(cfg, pix, run):
    """[run() with the grade gamma one ulp down, one ulp up] for a stop whose gamma is the device's powf; [] otherwise."""
    out = []
    if device_powf(cfg, pix):
        for direction in (-1, +1):
            with powf_nudged(direction):
                out.append(run())
    return out


# ---- the api route ----------------------------------------------------------------------------------------------------------------------
def api_call(env, stop, size, pix):
    pc, effects = env
    h, w = ct.SIZES[size]
    cfg, kw, inp = stop.config(), ct.api_keywords(stop, h, w), inputs(size, pix)
    m = masks(pc, stop, size, pix)
    per = dict(time_sec=ct.TIME_SEC, noise_seed=SEED, frame_index=FIRST)
    img = pc.apply_static_effects(*ct.static_args(inp["frame"], m, cfg), **per, **kw)
    eng = effects._engine(device(), h, w, pix_fmt(pix))
    plan_static = eng.last_plan()
    out, st = pc.apply_crt_effect(*ct.crt_args(inp["frame"], m, cfg, PERSISTENCE, inp["state"].copy()), **per, **kw)
    return dict(image=img, frame=out, state=np.array(st), plan_static=plan_static, plan_preview=eng.last_plan())


def api_anchor(env, stop, size, pix, res):
    pc, effects = env
    h, w = ct.SIZES[size]
    cfg, kw, inp = stop.config(), ct.api_keywords(stop, h, w), inputs(size, pix)
    m = masks(orc, stop, size, pix)
    planes = export_planes(effects._engine(device(), h, w, pix_fmt(pix)), cfg, h, w, [FIRST])
    per = dict(time_sec=ct.TIME_SEC, noise_plane=None if planes is None else planes[0])

    def run():
        exp = orc.apply_static_effects(*ct.static_args(inp["frame"], m, cfg), **per, **kw)
        uo, so = orc.apply_crt_effect(*ct.crt_args(inp["frame"], m, cfg, PERSISTENCE, inp["state"]), **per, **kw)
        return exp, uo, so
    exp, uo, so = run()
    var = oracle_variants(cfg, pix, run)
    exact = cfg["warp_strength"] == 0.0 and cfg["gamma"] == 1.0
    miss = [float_miss(res["image"], exp, 0.0 if exact else 3e-7, "float image", [v[0] for v in var]),
            float_miss(res["state"], so, 4e-7, "preview state", [v[2] for v in var]),
            half_miss(res["frame"], so, "half frame") if pix == "half" else u8_miss(res["frame"], uo, "uint8 frame")]
    return "; ".join(x for x in miss if x) or None


# ---- the loop route ---------------------------------------------------------------------------------------------------------------------
def render_settings(stop):
    from pythoncrt_amd.pipeline import RenderSettings
    return RenderSettings(**stop.config())


def new_pipeline(stop, size, pix):
    from pythoncrt_amd.pipeline import FramePipeline
    h, w = ct.SIZES[size]
    return FramePipeline(device(), h, w, render_settings(stop), fps=FPS, noise_seed=SEED, dtype=torch.float16 if pix == "half" else torch.uint8)


def loop_call(pipe, size, pix):
    h, w = ct.SIZES[size]
    inp = inputs(size, pix)
    dev = device()
    frames = torch.from_numpy(inp["clip"].copy()).to(dev)
    keep = torch.empty((N, h, w, 3), dtype=torch.float32, device=dev)
    out, st = pipe.run(frames, first_index=FIRST, state=torch.from_numpy(inp["state"].copy()).to(dev), local_states=keep)
    plan = pipe.plan()
    out2, st2 = pipe.run(frames, first_index=FIRST, state=torch.from_numpy(inp["state"].copy()).to(dev))      # the state stays in registers across a run
    return dict(frames=out.cpu().numpy(), state=st.cpu().numpy(), local_states=keep.cpu().numpy(), plan=plan,
                frames_in_registers=out2.cpu().numpy(), state_in_registers=st2.cpu().numpy(), plan_in_registers=pipe.plan())


LOOP_PARAMS = ("scanline_strength", "triad_gamma", "triad_preserve_luma", "aberration_px", "bloom_sigma", "bloom_strength", "bloom_threshold",
               "noise_strength", "scanline_period_px", "fast_bloom", "pixel_size", "glitch_amp_px", "glitch_height_frac", "brightness", "contrast",
               "gamma", "saturation", "temperature", "flicker_strength", "flicker_hz", "grain_size", "scanline_angle", "scanline_thickness",
               "warp_strength")


def loop_anchor(pipe, stop, size, pix, res):
    h, w = ct.SIZES[size]
    cfg, inp = stop.config(), inputs(size, pix)
    planes = export_planes(pipe.engine, cfg, h, w, range(FIRST, FIRST + N))
    params = {k: cfg[k] for k in LOOP_PARAMS}
    tail = (FPS, cfg["scanline_speed_px_s"], PERSISTENCE, cfg["triad_strength"], cfg["triad_softness"], cfg["vignette_strength"])
    miss = []
    if pix == "u8":
        run = lambda: orc.process_frames(list(inp["clip"]), params, *tail, noise_planes=planes, first_index=FIRST, prev_state=inp["state"])      # noqa: E731
        exp, exp_state = run()
        for key in ("frames", "frames_in_registers"):
            miss.append(u8_miss(res[key], np.stack(exp), key))
    else:
        def run(check=False):
            st = inp["state"]
            for j in range(N):
                _, st = orc.process_frames([inp["clip"][j]], params, *tail, noise_planes=None if planes is None else [planes[j]], first_index=FIRST + j,
                                           prev_state=st)
                for key in ("frames", "frames_in_registers") if check else ():
                    miss.append(half_miss(res[key][j], st, f"{key}[{j}]"))
            return None, st
        _, exp_state = run(check=True)
    var = [v[1] for v in oracle_variants(cfg, pix, run)]
    for key in ("state", "state_in_registers"):
        miss.append(float_miss(res[key], exp_state, 1e-6, key, var))
    return "; ".join(x for x in miss if x) or None


# ---- fresh results, once per (route, stop, size, format) ----------------------------------------------------------------------------------
def fresh(env, route, name, size, pix):
    key = (route, name, size, pix)
    if key not in FRESH:
        _, effects = env
        stop = ct.BY_NAME[name]
        if route == "api":
            saved, effects._tls.engines = effects._tls.engines, {}
            try:
                res = api_call(env, stop, size, pix)
                res["anchor"] = api_anchor(env, stop, size, pix, res)
            finally:
                effects._tls.engines = saved
        else:
            pipe = new_pipeline(stop, size, pix)
            res = loop_call(pipe, size, pix)
            res["anchor"] = loop_anchor(pipe, stop, size, pix, res)
        FRESH[key] = res
    return FRESH[key]


def compare(got, want, where):
    """Every piece of a reused ctx's result against the fresh ctx's: arrays bit for bit, plans as dicts."""
    bad = []
    for k, v in got.items():
        if isinstance(v, dict):
            if v != want[k]:
                bad.append(f"{k}: reused {v} != fresh {want[k]}")
        elif v.dtype != want[k].dtype or not np.array_equal(v, want[k]):
            n = int((v != want[k]).sum()) if v.shape == want[k].shape else -1
            d = float(np.abs(v.astype(np.float64) - want[k].astype(np.float64)).max()) if n >= 0 else float("nan")
            bad.append(f"{k}: {n} of {v.size} samples differ from the fresh ctx's, max |d| = {d:.3e}")
    assert not bad, f"{where}:\n  " + "\n  ".join(bad)


def check_family(stop, route, pix, size, res, where):
    key, prefix = stop.family_for(route, pix, size)
    plan = res["plan_static" if route == "api" else "plan"]
    assert str(plan.get(key, "")).startswith(prefix), f"{where}: the fresh plan {plan} does not land on {key}={prefix}"
    assert res["anchor"] is None, f"{where}: the fresh ctx's result misses the oracle: {res['anchor']}"


CASES = [(size, pix, route, walk) for size in ct.SIZES for pix in ct.PIXES for route in ct.ROUTES for walk in ct.WALKS]


@pytest.mark.parametrize("size,pix,route,walk", CASES, ids=["-".join(c) for c in CASES])
def test_reused_ctx_equals_fresh_ctx(env, size, pix, route, walk):
    _, effects = env
    names = ct.WALKS[walk](route, pix)
    try:
        if route == "api":
            cache = {}                                  # the engine cache of this walk: ONE Engine of this size and format lives in it
        else:
            pipe = new_pipeline(ct.BY_NAME[names[0]], size, pix)
        prev = None
        for i, name in enumerate(names):
            stop = ct.BY_NAME[name]
            where = f"{walk} walk, step {i}: {prev} -> {name} ({route}, {pix}, {ct.SIZES[size]})"
            want = fresh(env, route, name, size, pix)
            check_family(stop, route, pix, size, want, where)
            if route == "api":
                saved, effects._tls.engines = effects._tls.engines, cache
                try:
                    got = api_call(env, stop, size, pix)
                finally:
                    effects._tls.engines = saved
                assert len(cache) == 1
            else:
                if i:
                    pipe.set_settings(render_settings(stop))
                got = loop_call(pipe, size, pix)
            compare(got, {k: want[k] for k in got}, where)
            STEPS_RUN[0] += 1
            prev = name
    except (RuntimeError, OSError) as e:          # a HIP error: nothing more is started on a device that reported one
        pytest.exit(f"{size}-{pix}-{route}-{walk}: {type(e).__name__}: {e}", returncode=3)
    print(f"steps run so far: {STEPS_RUN[0]}")


def test_threaded_state_across_stops_and_a_resize(env):
    """12 GUI ticks of apply_crt_effect with numpy frames: the returned DeviceState goes back in as state_prev, every tick uses another stop
    of the random walk, tick 6 another frame size (crtfx_resize_state on the way in and on the way back).  Against the oracle threaded the
    same way (test_apply_crt_effect_sequence's / test_state_prev_of_another_size's bars: state <= 4e-7, uint8 <= 1 LSB on < 1e-3), and bit
    for bit against the same ticks with a ctx created for each tick (fed the reused chain's own incoming state)."""
    pc, effects = env
    names = ct.random_walk("api", "u8")[1:13]
    reused, sg, so = {}, None, None
    for tick, name in enumerate(names):
        stop, size = ct.BY_NAME[name], ("odd" if tick == 6 else "even")
        h, w = ct.SIZES[size]
        cfg, kw = stop.config(), ct.api_keywords(stop, h, w)
        frame = ct.make_frame(h, w, 40 + tick)
        per = dict(time_sec=tick / 30.0, noise_seed=SEED, frame_index=tick)
        state_in = None if sg is None else np.array(sg)
        effects._tls.engines = reused
        ug, sg = pc.apply_crt_effect(*ct.crt_args(frame, masks(pc, stop, size, "u8"), cfg, PERSISTENCE, sg), **per, **kw)
        effects._tls.engines = {}
        uf, sf = pc.apply_crt_effect(*ct.crt_args(frame, masks(pc, stop, size, "u8"), cfg, PERSISTENCE, state_in), **per, **kw)
        planes = export_planes(effects._engine(device(), h, w, pix_fmt("u8")), cfg, h, w, [tick])
        effects._tls.engines = {}
        where = f"tick {tick}: {names[tick - 1] if tick else None} -> {name} at {h} x {w}"
        assert np.array_equal(ug, uf) and np.array_equal(np.asarray(sg), np.asarray(sf)), f"{where}: the reused ctx differs from a fresh one"
        uo, so = orc.apply_crt_effect(*ct.crt_args(frame, masks(orc, stop, size, "u8"), cfg, PERSISTENCE, so), time_sec=tick / 30.0,
                                      noise_plane=None if planes is None else planes[0], **kw)
        err = float(np.abs(np.asarray(sg).astype(np.float64) - so).max())
        d = np.abs(ug.astype(np.int16) - uo.astype(np.int16))
        print(f"{where}: state err {err:.2e}, uint8 off {float((d != 0).mean()):.2e}")
        assert err <= 4e-7, (where, err)
        assert d.max() <= 1 and (d != 0).mean() < 1e-3, (where, int(d.max()), float((d != 0).mean()))
    assert len(reused) == 2


# ---- the Python-side mask caches ----------------------------------------------------------------------------------------------------------
MASK_HW = (40, 200)


def plane_args(frame, tm, vg):
    """No warp: the per-pixel-plane parity tests' bar is equality with float32(oracle) (tests/test_parity_gpu.py)."""
    return (frame, 0.6, tm, 2.2, True, 1, 1.2, 0.25, 0.0, 0.0, vg, 2.0, 1.0, False, 1, 0, 0.0)


def unsampled_element(shape):
    """An element effects._fingerprint does not visit: row 1 and column 1 are off its strides whenever the strides exceed 1."""
    rs, cs = max(1, shape[0] // 8), max(1, shape[1] // 64)
    assert rs > 1 and cs > 1 and 1 % rs != 0 and 1 % cs != 0
    return (1, 1)


@pytest.mark.parametrize("which", ["triad", "vignette"])
def test_plain_array_plane_edited_in_place(env, which):
    """A per-pixel plane handed in as a plain array and edited IN PLACE between two calls — at an element the strided sample of
    effects._fingerprint does not visit, then at [0, 0] — is read again, as the reference reads it on every call."""
    pc, effects = env
    from pythoncrt_amd import effects as fx
    h, w = MASK_HW
    frame = ct.make_frame(h, w, 50)
    tm, vg = ct.plane_masks(h, w, 51)
    a = lambda: plane_args(frame, tm if which == "triad" else None, vg if which == "vignette" else None)      # noqa: E731
    arr = tm if which == "triad" else vg
    effects._tls.engines = {}
    first = pc.apply_static_effects(*a())
    assert np.array_equal(first, orc.apply_static_effects(*a()).astype(np.float32))
    y, x = unsampled_element(arr.shape)
    for idx in ((y, x), (0, 0)):
        before = fx._fingerprint(arr)
        arr[idx] = arr[idx] * 0.25
        if idx != (0, 0):
            assert fx._fingerprint(arr) == before, "the element is sampled after all"
        got = pc.apply_static_effects(*a())
        exp = orc.apply_static_effects(*a()).astype(np.float32)
        assert not np.array_equal(exp, first), "the edit does not change the oracle's image"
        assert np.array_equal(got, exp), f"{which} plane edited in place at {idx}: {int((got != exp).sum())} samples differ from the oracle; the device kept the old plane"
        first = exp
    assert len(effects._tls.engines) == 1
    effects._tls.engines = {}


def test_tensor_mask_edited_in_place(env):
    """A device-tensor mask edited in place: its _version moves and the edit is seen."""
    pc, effects = env
    h, w = MASK_HW
    frame = ct.make_frame(h, w, 52)
    tm, _ = ct.plane_masks(h, w, 53)
    t = torch.from_numpy(tm.copy()).to(device())
    effects._tls.engines = {}
    g0 = pc.apply_static_effects(*plane_args(frame, t, None))
    assert np.array_equal(g0, orc.apply_static_effects(*plane_args(frame, tm, None)).astype(np.float32))
    v0 = t._version
    t[1, 1] *= 0.25
    tm2 = tm.copy()
    tm2[1, 1] *= np.float32(0.25)
    assert t._version > v0
    g1 = pc.apply_static_effects(*plane_args(frame, t, None))
    assert np.array_equal(g1, orc.apply_static_effects(*plane_args(frame, tm2, None)).astype(np.float32)) and not np.array_equal(g1, g0)
    effects._tls.engines = {}


def test_recognised_arrays_in_rotation_and_rebuilt_in_place(env):
    """Five reference-built mask pairs in rotation — one more than the recognition cache holds — on one engine cache: every call equals the call on a fresh
    ctx.  Then one recognised pair is rebuilt in place with another strength (np.copyto): the rebuild is seen."""
    pc, effects = env
    from pythoncrt_amd import effects as fx
    h, w = MASK_HW
    frame = ct.make_frame(h, w, 54)
    strengths = [(0.2, 0.0, 0.1), (0.35, 0.5, 0.25), (0.5, 1.0, 0.4), (0.7, 1.4, 0.6), (0.9, 0.3, 1.0)]
    assert len(strengths) == fx._RECOGNISED_MAX + 1
    arrays = [(orc.make_triad_mask(h, w, s, soft), orc.make_vignette(h, w, v)) for s, soft, v in strengths]
    a = lambda tm, vg: (frame, 0.6, tm, 2.2, False, 1, 3.0, 0.25, 0.0, 1.5, vg, 2.0, 1.0, False, 1, 0, 0.0)      # noqa: E731
    kw = dict(noise_seed=SEED, frame_index=1, warp_strength=0.15)
    want = []
    for tm, vg in arrays:
        effects._tls.engines = {}
        want.append(pc.apply_static_effects(*a(tm.copy(), vg.copy()), **kw))
    assert all(not np.array_equal(want[0], x) for x in want[1:])
    reused = effects._tls.engines = {}
    for turn in range(3 * len(arrays)):
        k = turn % len(arrays)
        got = pc.apply_static_effects(*a(*arrays[k]), **kw)
        assert np.array_equal(got, want[k]), f"turn {turn}: mask pair {k} on the reused ctx differs from a fresh ctx"
        assert len(fx._RECOGNISED) <= fx._RECOGNISED_MAX and "triad_full" not in reused[next(iter(reused))].keep
    assert len(reused) == 1 and len(reused) <= fx._ENGINES_PER_THREAD
    tm, vg = arrays[1]
    pc.apply_static_effects(*a(tm, vg), **kw)
    np.copyto(tm, arrays[3][0])
    np.copyto(vg, arrays[3][1])
    got = pc.apply_static_effects(*a(tm, vg), **kw)
    assert np.array_equal(got, want[3]), "a recognised pair rebuilt in place with another strength: the device kept the old masks"
    effects._tls.engines = {}
