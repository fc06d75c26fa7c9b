"""CPU: the model of the pointwise render chain (tests/warp_model.point_render: the oracle's chain with the warp off, the persistence state
stored as float32, its parameter list widened to the colour grade, flicker, coarse grain and the 2-D scanline plane) tied to the unmodified
oracle, and the table tests/point_builds.py tied to the restated launcher — without a device.

  * persistence 0: the model's uint8 frames ARE the oracle's (the float32 narrowing in front of the quantiser is the oracle's own);
  * persistence on: the model differs from the oracle by the float32 storage of the state alone — within the bars the suite states for
    that (uint8 <= 1 LSB, state <= 1e-6);
  * every row's settings produce, through default_point_plan on every shape the row runs on, exactly the plan strings the row asserts on
    the GPU, and those strings name exactly the row's instances."""
import dataclasses

import numpy as np
import pytest

from oracle import crt_oracle as orc
from tests import point_builds as pb
from tests import warp_model as wm

FPS, FIRST = 25.0, 7
# a handful of the table's settings: the defaults with and without pixelate, one of each grade form, a flicker (promotes), coarse grain, stages off
TIE_ROWS = ("fused_fast_u8_pix_none", "fused_fast_u8_none", "fused_gradelut_u8_none", "fused_grade_u8_pix_none", "fused_flicker_u8_none",
            "fused_coarse_u8_pix_none", "fused_scan2d_u8_none", "lean_runtime_a_u8_none", "lean_runtime_b_u8_none", "lean_nobloom_u8_none")


def cfg_of(row, persistence):
    return dict(pb.DEFAULTS, **row.settings, persistence=persistence)


def planes_for(cfg, h, w, n, seed):
    if cfg["noise_strength"] <= 0.0:
        return None
    g = cfg["grain_size"]
    gh, gw = (h, w) if g <= 1 else (max(1, h // g), max(1, w // g))
    return [wm.make_plane(gh, gw, seed + j) for j in range(n)]


def test_defaults_are_the_render_settings_defaults():
    pytest.importorskip("torch")
    from pythoncrt_amd.pipeline import RenderSettings
    assert {f.name: f.default for f in dataclasses.fields(RenderSettings)} == pb.DEFAULTS


def test_model_parameters_cover_the_grain_tests_key_list():
    keys = ("scanline_strength", "triad_gamma", "triad_preserve_luma", "aberration_px", "bloom_sigma", "bloom_strength", "bloom_threshold",
            "noise_strength", "scanline_period_px", "fast_bloom", "pixel_size", "glitch_amp_px", "glitch_height_frac", "brightness", "contrast",
            "gamma", "saturation", "temperature", "flicker_strength", "flicker_hz", "grain_size", "scanline_angle", "scanline_thickness",
            "warp_strength")          # tests/test_grain_gpu.PARAM_KEYS (that module needs torch)
    assert sorted(wm._params(pb.DEFAULTS)) == sorted(keys)


@pytest.mark.parametrize("name", TIE_ROWS)
@pytest.mark.parametrize("hw", [(34, 66), (37, 131)])
def test_model_equals_the_oracle_without_persistence(name, hw):
    h, w = hw
    cfg = cfg_of(pb.BY_NAME[name], 0.0)
    frames = [wm.make_frame(h, w, 40 + j) for j in range(3)]
    planes = planes_for(cfg, h, w, 3, 90)
    got, states = wm.point_render(frames, cfg, False, FPS, FIRST, planes)
    exp, _ = orc.process_frames(frames, wm._params(cfg), FPS, cfg["scanline_speed_px_s"], 0.0, cfg["triad_strength"], cfg["triad_softness"],
                                cfg["vignette_strength"], noise_planes=planes, first_index=FIRST)
    for j in range(3):
        assert np.array_equal(got[j], exp[j]), (name, j)
        assert states[j].dtype == np.float32 and got[j].dtype == np.uint8


@pytest.mark.parametrize("name", TIE_ROWS)
def test_model_differs_from_the_oracle_by_the_float32_state_alone(name):
    h, w = 34, 66
    row = pb.BY_NAME[name]
    for p in (0.2, 0.9):
        cfg = cfg_of(row, p)
        frames = [wm.make_frame(h, w, 60 + j) for j in range(5)]
        planes = planes_for(cfg, h, w, 5, 70)
        got, states = wm.point_render(frames, cfg, False, FPS, FIRST, planes)
        exp, exp_states = wm.oracle_render(frames, cfg, FPS, FIRST, planes)
        assert np.array_equal(got[0], exp[0])                     # the first frame passes through unblended
        for j in range(5):
            d = np.abs(got[j].astype(np.int16) - exp[j].astype(np.int16))
            assert d.max() <= 1 and (d != 0).mean() < 1e-3, (name, p, j, int(d.max()), float((d != 0).mean()))
            assert np.abs(states[j].astype(np.float64) - exp_states[j]).max() <= 1e-6, (name, p, j)


def test_injected_scan_plane_is_an_input_not_arithmetic():
    """The oracle's own 2-D scanline mask handed back in gives the oracle's own frames; a changed plane changes them."""
    h, w = 10, 12
    cfg = cfg_of(pb.BY_NAME["fused_scan2d_u8_none"], 0.0)
    frames = [wm.make_frame(h, w, 5)]
    planes = planes_for(cfg, h, w, 1, 6)
    own = orc.make_scanline_mask_2d(h, w, cfg["scanline_strength"], cfg["scanline_period_px"], (FIRST / FPS) * cfg["scanline_speed_px_s"],
                                    cfg["scanline_angle"], cfg["scanline_thickness"])
    a, _ = wm.point_render(frames, cfg, False, FPS, FIRST, planes)
    b, _ = wm.point_render(frames, cfg, False, FPS, FIRST, planes, scan_planes=[own])
    c, _ = wm.point_render(frames, cfg, False, FPS, FIRST, planes, scan_planes=[own * np.float32(0.5)])
    assert np.array_equal(a[0], b[0]) and not np.array_equal(a[0], c[0])
    assert orc.make_scanline_mask_2d(2, 2, 0.0, 2.0, 0.0, 0.0, 1.0).shape == (2, 2)      # and the oracle's function is back in place


@pytest.mark.parametrize("name", [r.name for r in pb.ROWS])
def test_row_settings_land_on_the_rows_build(name):
    row = pb.BY_NAME[name]
    shapes = pb.row_shapes(row)
    assert len(shapes) >= 3 and {"tiny", "ragged", "strips"} <= set(shapes) and (("odd" in shapes) == (row.shapes == "any")), (name, shapes)
    frames, float_out = (4, False) if row.route == "loop" else (1, row.route == "api")
    for k in shapes:
        h, w = pb.SHAPES[k]
        plan = pb.default_point_plan(row.settings, row.pix, h, w, row.options, row.blend, frames, float_out)
        assert plan["point"] == row.point and plan.get("half", "") == row.half, (name, k, plan)
        assert (pb.plan_instance(plan["point"]),) + ((pb.plan_instance(plan["half"]),) if "half" in plan else ()) == row.kernels
    assert row.settings.get("gamma", 1.0) == 1.0 and "persistence" not in row.settings and row.settings.get("warp_strength", 0.0) == 0.0
    if row.point.startswith("k_point_fused_seq<"):
        assert row.shapes == "even" and not row.half
        # the same settings where the fused kernel cannot run (an odd size) stay on a lean or general sequence build
        assert pb.default_point_plan(row.settings, row.pix, 37, 131, row.options, row.blend, 4)["point"].startswith(("k_point_lean_seq<", "k_point_sel_seq<"))


def test_the_gamma_cases_name_one_row_per_grade_family():
    fams = sorted(r.gamma_family for r in pb.ROWS if r.gamma_family)
    assert fams == ["+grade half", "+grade u8", "+gradelut", "runtime"]
    for r in pb.ROWS:
        if r.gamma_family:         # with a gamma on top the row stays on its build
            plan = pb.default_point_plan(dict(r.settings, gamma=1.8), r.pix, 50, 198, r.options, r.blend, 4)
            assert plan["point"] == r.point, (r.name, plan)


def test_planner_restatement_on_known_settings():
    """default_point_plan against plan strings the GPU suite already pins (tests/test_fullsize_gpu.py, tests/test_parity_gpu.py)."""
    P = lambda s, pix="u8", h=72, w=128, o=None, blend="render": pb.default_point_plan(s, pix, h, w, o, blend, 4)      # noqa: E731
    assert P({}) == {"point": "k_point_fused_seq<fast+pixelate,u8,render>"}
    assert P({}, h=71) == {"point": "k_point_lean_seq<fast+pixelate,u8,render>", "half": "k_half_group<fast+pixelate,u8>"}
    assert P(dict(bloom_strength=0.0))["point"] == "k_point_lean_seq<fast+pixelate-bloom,u8,render>"
    assert P(dict(bloom_strength=0.0), "half")["point"] == "k_point_lean_seq<runtime,half,render>"
    assert P(dict(grain_size=2), "half")["point"] == "k_point_sel_seq<half,two-round>"
    assert P(dict(grain_size=3, pixel_size=1), blend="none")["point"] == "k_point_fused_seq<fast+coarse,u8,none>"
    assert P(dict(scanline_angle=10.0))["point"] == "k_point_fused_seq<fast+pixelate+scan2d,u8,render>"
    assert P(dict(bloom_threshold=0.3), blend="none")["point"] == "k_point_fused_seq<fast+pixelate,u8,none>"
    assert P(dict(saturation=1.2))["point"] == "k_point_fused_seq<fast+pixelate+sat,u8,render>"
    assert P(dict(saturation=1.2), o={"NO_FUSED_HALF": 1})["point"] == "k_point_lean_seq<fast+pixelate+grade,u8,render>"
    assert P(dict(saturation=1.2), "half")["point"] == "k_point_fused_seq<fast+pixelate+grade,half,render>"
    assert P(dict(brightness=0.05, contrast=1.1))["point"] == "k_point_fused_seq<fast+pixelate+gradelut,u8,render>"
    assert P(dict(vignette_strength=0.0, noise_strength=0.0))["point"] == "k_point_fused_seq<runtime,u8,render>"
    assert P({}, o={"FORCE_RUNTIME_FLAGS": 1}) == {"point": "k_point_sel_seq<u8,two-round>", "half": "k_half_group<runtime,any>"}
    assert P({}, o={"POINT_TILES": 16})["point"] == "k_point_lean_seq<fast+pixelate,u8,render>"
    several = dict(saturation=1.2, bloom_threshold=0.3, flicker_strength=0.2, flicker_hz=9.0, pixel_size=1)
    assert P(several, h=1080, w=1920)["point"] == "k_point_fused_seq<fast+grade,u8,render>"
    assert P(dict(brightness=0.05, contrast=1.1, gamma=1.2, temperature=-0.2), h=1080, w=1920)["point"] == "k_point_fused_seq<fast+pixelate+gradelut,u8,render>"
    one = pb.default_point_plan({}, "u8", 72, 128, None, "none", 1)
    assert one == {"point": "k_point_lean<fast+pixelate,u8,none>", "half": "k_half<fast+pixelate,u8>"}
