"""The interlace stage without a GPU (include/crtfx_interlace.h): the model against a per-pixel restatement of the header and a float64
restatement of the two filters, its properties (constants survive, rows kept as bits, the two orders, the odd tail, COMPLEX's clamp rule, the
half quantiser, the accumulator bounds, the smallest heights, the round trip with the deinterlace model), the C-ABI bound symbol for symbol
and refusing bad arguments before it touches a device, every refusal of process_frames(deliver_interlace=) and of the CLI's flags, the
stages and counts of DeliveryEnd with and without the keyword, and the builds' registers against the header."""
import ctypes
import itertools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pythoncrt_amd import _lib, _stage, canvas, depth, ends, formats, ingest, interlace, lut3d, resample, resize16  # noqa: E402
from tests import deint_model  # noqa: E402
from tests import interlace_model as model  # noqa: E402
from tests import resize16_model  # noqa: E402

HEADER = os.path.join(ROOT, "include", "crtfx_interlace.h")
DTYPES = (np.uint8, np.float16)
COMBOS = list(itertools.product(model.ORDERS, model.LOWPASS))


def _all_halves():
    return np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)


def _source(dtype, shape, seed):
    """Noise: bytes; or halves across every rule — quarter codes, values between them and past both ends, NaN, infinities, -0."""
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    f = (rng.integers(-40, 8 * 1030, shape) / 32.0).astype(np.float16)
    flat = f.reshape(-1)
    pick = rng.integers(0, flat.size, max(1, flat.size // 16))
    flat[pick] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0, 255.5, 254.875, 0.125, 6e-8, 65504.0], dtype=np.float16), pick.size)
    return f


# ---- the arithmetic -------------------------------------------------------------------------------------------------------------------------

def _code(sample):
    """One sample's integer, from the header's words (not through the model)."""
    if isinstance(sample, np.uint8):
        return int(sample)
    f = float(sample)
    if f != f:
        return 0
    t = min(max(4.0 * f, 0.0), 1020.0)
    lo = int(np.floor(t))
    frac = t - lo
    return lo + (1 if frac > 0.5 or (frac == 0.5 and lo % 2 == 1) else 0)


def _per_pixel(frames, order, lowpass):
    """The header, one sample at a time."""
    n, h, w, _ = frames.shape
    half = frames.dtype == np.float16
    top = 1020 if half else 255
    out = np.zeros(((n + 1) // 2, h, w, 3), dtype=frames.dtype)
    out_bits = model.bits(out)
    for j in range(out.shape[0]):
        fa, fb = 2 * j, min(2 * j + 1, n - 1)
        for y in range(h):
            f = frames[fa if y % 2 == (0 if order == "tff" else 1) else fb]
            for x in range(w):
                for k in range(3):
                    def r(d):
                        return _code(f[min(max(y + d, 0), h - 1), x, k])
                    if lowpass == "none":
                        out_bits[j, y, x, k] = model.bits(f)[y, x, k]       # as bits: a NaN keeps its payload
                        continue
                    if lowpass == "linear":
                        v = (r(-1) + 2 * r(0) + r(1) + 2) >> 2
                    else:
                        v = (-r(-2) + 2 * r(-1) + 6 * r(0) + 2 * r(1) - r(2) + 4) >> 3
                        v = min(max(v, 0), top)
                        v = max(v, r(0)) if r(-1) + r(1) > 2 * r(0) else min(v, r(0))
                    out[j, y, x, k] = np.float16(v / 4.0) if half else v
    return out


def test_names_are_one_list_in_the_model_and_the_module():
    assert interlace.ORDERS == model.ORDERS == ("tff", "bff") and interlace.LOWPASS == model.LOWPASS == ("none", "linear", "complex")
    assert interlace.Interlace.frames_in == 2 and interlace.Interlace.frames_out == 1 and _stage.FramePlan.frames_in == 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order,lowpass", COMBOS)
def test_model_against_the_header_per_pixel(dtype, order, lowpass):
    for (h, w), n in (((2, 3), 3), ((3, 2), 2), ((4, 3), 1), ((7, 4), 5)):
        src = _source(dtype, (n, h, w, 3), [h, w, n])
        got = model.interlace(src, order, lowpass)
        assert got.dtype == dtype and got.shape == ((n + 1) // 2, h, w, 3)
        assert np.array_equal(model.bits(got), model.bits(_per_pixel(src, order, lowpass))), (h, w, n)
    assert model.interlace(src[:0], order, lowpass).shape == (0, 7, 4, 3)


@pytest.mark.parametrize("dtype", DTYPES)
def test_model_against_float64_filters(dtype):
    """(s + 2) >> 2 is floor(s / 4 + 1 / 2) and (s + 4) >> 3 is floor(s / 8 + 1 / 2): exact in float64 at these sizes."""
    src = model.noise(9, 11, n=1, dtype=dtype, seed=2)[0]
    c = model.codes(src).astype(np.float64)
    h = 9
    r = {k: c[np.clip(np.arange(h) + k, 0, h - 1)] for k in (-2, -1, 0, 1, 2)}
    lin = np.floor((r[-1] + 2 * r[0] + r[1]) / 4 + 0.5)
    assert np.array_equal(model.codes(model.filtered(src, "linear")), lin.astype(np.int64))
    v = np.floor((-r[-2] + 2 * r[-1] + 6 * r[0] + 2 * r[1] - r[2]) / 8 + 0.5)
    v = np.minimum(np.maximum(v, 0), model.top(dtype))
    cx = np.where(r[-1] + r[1] > 2 * r[0], np.maximum(v, r[0]), np.minimum(v, r[0]))
    assert np.array_equal(model.codes(model.filtered(src, "complex")), cx.astype(np.int64))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order,lowpass", COMBOS)
def test_a_constant_frame_is_unchanged(dtype, order, lowpass):
    for h, w in ((2, 1), (3, 7), (8, 16)):
        src = np.empty((3, h, w, 3), dtype=dtype)
        src[...] = np.array([17, 200.25 if dtype == np.float16 else 200, 255], dtype=dtype)
        out = model.interlace(src, order, lowpass)
        assert out.shape == (2, h, w, 3) and (out == src[0, 0, 0]).all()
        src[...] = np.array([0, 255, 0], dtype=dtype)                           # both ends of the scale: COMPLEX's clamps are not needed
        assert np.array_equal(model.bits(model.interlace(src, order, lowpass)), model.bits(src[:2]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_none_keeps_rows_as_bits_from_the_right_frame(dtype):
    src = _source(dtype, (4, 9, 12, 3), 3)
    if dtype == np.float16:                                                     # patterns the arithmetic would change: NaNs with payloads, -0, negatives, > 255
        src.view(np.uint16)[:, :, :4, :] = np.array([0x7e01, 0xfc01, 0x8000, 0xc500, 0x7bff, 0x0001, 0x7c00, 0xfe55, 0x3555, 0x5bf9, 0x5c01, 0x7fff],
                                                    dtype=np.uint16).reshape(4, 3)
    for order in model.ORDERS:
        first = model.ORDERS.index(order)
        out = model.interlace(src, order, "none")
        for j in range(2):
            assert np.array_equal(model.bits(out[j, first::2]), model.bits(src[2 * j, first::2]))
            assert np.array_equal(model.bits(out[j, 1 - first::2]), model.bits(src[2 * j + 1, 1 - first::2]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lowpass", model.LOWPASS)
def test_tff_on_a_b_is_bff_on_b_a_and_the_odd_tail_is_woven_with_itself(dtype, lowpass):
    src = _source(dtype, (5, 6, 5, 3), 8)
    a, b = src[0], src[1]
    assert np.array_equal(model.bits(model.weave(a, b, "tff", lowpass)), model.bits(model.weave(b, a, "bff", lowpass)))
    assert not np.array_equal(model.bits(model.weave(a, b, "tff", lowpass)), model.bits(model.weave(a, b, "bff", lowpass)))
    for order in model.ORDERS:
        out = model.interlace(src, order, lowpass)
        assert out.shape[0] == 3
        assert np.array_equal(model.bits(out[2]), model.bits(model.weave(src[4], src[4], order, lowpass)))
        assert np.array_equal(model.bits(out[2]), model.bits(model.filtered(src[4], lowpass)))      # woven with itself: the frame, filtered
        assert np.array_equal(model.bits(out[:2]), model.bits(model.interlace(src[:4], order, lowpass)))
        assert np.array_equal(model.bits(out[2:]), model.bits(model.interlace(np.stack([src[4], src[4]]), order, lowpass)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_complex_stays_between_its_neighbours_and_both_clamps_and_branches_run(dtype):
    """Where r(-1) + r(1) > 2 r(0) the result is max(v, r(0)) >= r(0); else min(v, r(0)) <= r(0); and v itself, a [2 6 2] / 8 mean less an
    overshoot term, is bounded: the result lies in [min, max] of r(-1), r(0), r(1) whenever the rule took r(0)'s side of v, and always within
    0..M.  Driven: v < 0 before the clamp, v > M before it, and both branches with v on either side of r(0)."""
    top = model.top(dtype)
    src = model.noise(12, 40, n=1, dtype=dtype, seed=4)[0]
    src[0:5, 0] = model.from_codes(np.array([top, 0, 0, 0, top])[:, None].repeat(3, 1), dtype)         # row 2: acc = -2 top + 4 < 0
    src[0:5, 1] = model.from_codes(np.array([0, top, top, top, 0])[:, None].repeat(3, 1), dtype)       # row 2: acc = 10 top + 4 > 8 top
    c = model.codes(src)
    h = 12
    r = {k: c[np.clip(np.arange(h) + k, 0, h - 1)] for k in (-2, -1, 0, 1, 2)}
    acc = -r[-2] + 2 * r[-1] + 6 * r[0] + 2 * r[1] - r[2] + 4
    raw = acc >> 3
    assert raw.min() < 0 and raw.max() > top and acc[2, 0, 0] == -2 * top + 4 and acc[2, 1, 0] == 10 * top + 4
    out = model.codes(model.filtered(src, "complex"))
    assert out[2, 0, 0] == 0 and out[2, 1, 0] == top and out.min() >= 0 and out.max() <= top
    v = np.clip(raw, 0, top)
    up = r[-1] + r[1] > 2 * r[0]
    assert (up & (v > r[0])).any() and (up & (v < r[0])).any() and (~up & (v > r[0])).any() and (~up & (v < r[0])).any()
    assert (out[up] >= r[0][up]).all() and (out[~up] <= r[0][~up]).all()
    lo, hi = np.minimum(np.minimum(r[-1], r[0]), r[1]), np.maximum(np.maximum(r[-1], r[0]), r[1])
    held = out == r[0]                                                          # the rule took r(0): trivially between
    assert ((out >= lo) & (out <= hi))[held].all() and held.any() and (~held).any()


def test_the_half_quantiser_on_every_pattern_and_the_accumulator_bounds():
    halves = _all_halves()
    q = model.quantise(halves)
    assert np.array_equal(q, resize16_model.quantise(halves)) and np.array_equal(q, deint_model.quantise(halves))
    assert q.min() == 0 and q.max() == model.QMAX == 1020 and np.array_equal(q, [_code(v) for v in halves])
    back = model.from_codes(np.arange(1021), np.float16)                        # every quarter code is a half: nothing is rounded
    assert np.array_equal(back.astype(np.float64) * 4, np.arange(1021)) and np.array_equal(model.quantise(back), np.arange(1021))
    # all 65 536 patterns through the three settings: NONE keeps them, the filters give quarter codes whatever goes in
    w = 65536 // 3 + 1
    src = np.zeros((2, 5, w, 3), dtype=np.float16)
    for f, y in itertools.product(range(2), range(5)):
        src.view(np.uint16)[f, y].reshape(-1)[:65536] = np.roll(np.arange(65536, dtype=np.uint16), 7919 * (5 * f + y))
    assert np.array_equal(model.bits(model.interlace(src, "tff", "none")[0, 0::2]), model.bits(src[0, 0::2]))
    assert np.array_equal(model.bits(model.interlace(src, "tff", "none")[0, 1::2]), model.bits(src[1, 1::2]))
    for lowpass in ("linear", "complex"):
        out = model.interlace(src, "bff", lowpass)[0].astype(np.float64) * 4
        assert np.array_equal(out, np.rint(out)) and out.min() >= 0 and out.max() <= 1020
    # the accumulator: its two extremes, as the header states them, for both scales
    assert (model.ACC_MIN, model.ACC_MAX) == (-2040, 10204) == (-2 * 1020, 10 * 1020 + 4)
    ext = np.zeros((2, 5, 1, 3), dtype=np.float16)
    ext[0, (0, 4)] = 255.0                                                      # -r(-2) - r(2) alone
    ext[1, 1:4] = 255.0                                                         # 2 r(-1) + 6 r(0) + 2 r(1) alone
    model.interlace(ext, "tff", "complex")                                      # the model asserts the bounds
    hdr = open(HEADER).read()
    assert "-2040 .. 10204" in hdr and "-510 .. 2554" in hdr


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h", [2, 3, 4])
def test_the_smallest_heights(dtype, h):
    """h = 2, 3, 4: every clamped index occurs (y - 2, y - 1 below 0; y + 1, y + 2 past h - 1, both at once for h = 2 and 3)."""
    src = _source(dtype, (3, h, 5, 3), h)
    for order, lowpass in COMBOS:
        assert np.array_equal(model.bits(model.interlace(src, order, lowpass)), model.bits(_per_pixel(src, order, lowpass)))
    c = model.codes(src[0])
    assert np.array_equal(model.rows(c, -2)[0], c[0]) and np.array_equal(model.rows(c, 2)[h - 1], c[h - 1])
    assert np.array_equal(model.rows(c, -2)[1], c[0]) and np.array_equal(model.rows(c, 2)[h - 2], c[h - 1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", deint_model.METHODS)
def test_round_trip_with_the_deinterlace_model(dtype, method):
    src = _source(dtype, (3, 9, 12, 3), 12)
    for order in model.ORDERS:
        other = model.ORDERS[1 - model.ORDERS.index(order)]
        fields = deint_model.deinterlace(src, method, order, "both")
        assert fields.shape[0] == 6
        assert np.array_equal(model.bits(model.interlace(fields, order, "none")), model.bits(src))
        assert not np.array_equal(model.bits(model.interlace(fields, other, "none")), model.bits(src))


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------------------

_vp = ctypes.c_void_p
SIGNATURES = {
    "crtfx_interlace_create": (ctypes.c_int, [ctypes.c_int] * 6 + [ctypes.POINTER(_vp)]),
    "crtfx_interlace_destroy": (ctypes.c_int, [_vp]),
    "crtfx_interlace_last_error": (ctypes.c_char_p, [_vp]),
    "crtfx_interlace_run": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_int, _vp]),
    "crtfx_interlace_set_option": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "crtfx_interlace_last_plan": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_size_t]),
    "crtfx_interlace_frames_in": (ctypes.c_int, [_vp]),
}


def test_symbols_are_bound_and_the_header_declares_them():
    assert _lib.INTERLACE_SYMBOLS == SIGNATURES and list(_lib.INTERLACE_SYMBOLS) == list(SIGNATURES) and _lib.INTERLACE_OPT_FORCE_GENERAL == 1
    assert _lib.INTERLACE_SYMBOLS == _lib.frame_symbols("interlace", [ctypes.c_int] * 5, frames_in=(ctypes.c_int, [_vp]))
    assert (_lib.INTERLACE_TFF, _lib.INTERLACE_BFF, _lib.INTERLACE_NONE, _lib.INTERLACE_LINEAR, _lib.INTERLACE_COMPLEX) == (0, 1, 0, 1, 2)
    lib = _lib.load()
    for name, (res, args) in SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res, name
    hdr = open(HEADER).read()
    for text in ("CRTFX_INTERLACE_OPT_FORCE_GENERAL = 1", "CRTFX_INTERLACE_TFF = 0", "CRTFX_INTERLACE_BFF = 1", "CRTFX_INTERLACE_NONE = 0",
                 "CRTFX_INTERLACE_LINEAR = 1", "CRTFX_INTERLACE_COMPLEX = 2", "NOT claimed is equality with ffmpeg's `interlace`",
                 "so they mix the two fields", "interlace=k_interlace<linear,u8,vec>;frames=6"):
        assert text in hdr, text
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(crtfx_interlace_\w+)\s*\(([^)]*)\)\s*;", hdr)}
    assert set(protos) == set(SIGNATURES) and len(protos) == 7, set(protos) ^ set(SIGNATURES)
    for name, args in protos.items():
        assert len(args.split(",")) == len(SIGNATURES[name][1]), name
    order = [a.split()[-1].lstrip("*") for a in protos["crtfx_interlace_create"].split(",")]
    assert order == ["device", "h", "w", "pix_fmt", "order", "lowpass", "out_plan"]
    others = set()
    for table in ("SYMBOLS", "INGEST_SYMBOLS", "EGRESS_SYMBOLS", "UNPACK_SYMBOLS", "DEEP_SYMBOLS", "YUV422_SYMBOLS", "DEEP444_SYMBOLS", "SITED_SYMBOLS",
                  "EGRESS_SITED_SYMBOLS", "RESIZE16_SYMBOLS", "RESAMPLE_SYMBOLS", "CANVAS_SYMBOLS", "DEPTH_SYMBOLS", "DEINT_SYMBOLS", "ADEINT_SYMBOLS",
                  "LUT3D_SYMBOLS"):
        others |= set(getattr(_lib, table))
    assert not set(SIGNATURES) & others
    assert all(os.path.basename(f) in {os.path.basename(s) for s in _lib.SOURCES} for f in ("crtfx_interlace.hip", "crtfx_interlace.h", "crtfx_frame_host.h"))
    assert all(os.path.exists(s) for s in _lib.SOURCES) and "crtfx_interlace" in _lib.STAGE_UNITS
    import pythoncrt_amd as pc
    assert pc.Interlace is interlace.Interlace and "Interlace" in pc.__all__
    assert issubclass(pc.Interlace, _stage.FramePlan) and issubclass(pc.Interlace, _stage.Handle)
    assert not issubclass(pc.Interlace, _stage.StagePlan) and not issubclass(pc.Interlace, _stage.ResizePlan)
    assert pc.Interlace._family == "interlace" and pc.Interlace._force_option == 1
    unit = open(os.path.join(_lib.CSRC, "crtfx_interlace.hip")).read()
    assert "namespace crtfx_interlace_impl" in unit and "crtfx_frames::run<U>" in unit and "hipGetDevice" not in unit      # run() is the skeleton's
    import bench                                                               # a namespace of its own, outside the chain's evidence hash
    assert "crtfx_interlace" not in open(bench.__file__).read()


GOOD = dict(device=0, h=9, w=24, pix_fmt=_lib.PIX_U8, order=_lib.INTERLACE_BFF, lowpass=_lib.INTERLACE_COMPLEX)


def _create(lib, no_out=False, **kw):
    a = dict(GOOD)
    a.update(kw)
    plan = ctypes.c_void_p(1)
    rc = lib.crtfx_interlace_create(*(a[k] for k in GOOD), None if no_out else ctypes.byref(plan))
    return rc, plan, (lib.crtfx_interlace_last_error(None) or b"").decode()


def test_create_refuses_bad_arguments_before_it_touches_a_device():
    """Every refusal of crtfx_interlace_create comes before the device is asked for, so it holds on any machine; *out_plan is NULL and the
    message names the offending field.  The call that passes every check is left with the device: `no HIP device 4096`."""
    lib = _lib.load()
    cases = [(dict(h=v), f"h = {v} outside 2..32767") for v in (1, 0, -3, 32768)] + [(dict(w=v), f"w = {v} outside 1..32767") for v in (0, -3, 32768)]
    cases += [({k: v}, f"unknown {k} {v}") for k in ("pix_fmt", "order") for v in (2, -1, 7)] + [(dict(lowpass=v), f"unknown lowpass {v}") for v in (3, -1, 7)]
    for kw, text in cases:
        rc, plan, msg = _create(lib, **kw)
        assert rc == _lib.E_INVALID and not plan.value and text in msg, (kw, rc, plan.value, msg)
    rc, plan, msg = _create(lib, no_out=True)
    assert rc == _lib.E_INVALID and "out_plan" in msg
    for kw in (dict(), dict(h=2, w=1), dict(h=32767, w=32767, pix_fmt=_lib.PIX_F16), dict(order=0, lowpass=0), dict(lowpass=1)):
        rc, plan, msg = _create(lib, device=4096, **kw)
        assert rc == _lib.E_HIP and not plan.value and "no HIP device 4096" in msg, (kw, rc, msg)
    assert lib.crtfx_interlace_destroy(None) == _lib.OK and lib.crtfx_interlace_set_option(None, 1, 1) == _lib.E_INVALID
    assert lib.crtfx_interlace_frames_in(None) == 0
    assert lib.crtfx_interlace_run(None, None, 0, None, 0, 1, None) == _lib.E_INVALID
    assert lib.crtfx_interlace_last_plan(None, ctypes.create_string_buffer(8), 8) == _lib.E_INVALID


def test_python_plan_refuses_before_a_device():
    for kw in (dict(order="top"), dict(lowpass="vlpf"), dict(order=None), dict(lowpass=2)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            interlace.Interlace("cpu", (4, 4), **kw)
    with pytest.raises(ValueError, match="ROCm device"):
        interlace.Interlace("cpu", (4, 4))


def test_frame_plan_sizes_its_output_from_frames_in():
    import torch

    class Pair(_stage.FramePlan):
        frames_in = 2
    for cls, frames_out, counts in ((Pair, 1, {0: 0, 1: 1, 2: 1, 3: 2, 5: 3, 8: 4}), (_stage.FramePlan, 2, {0: 0, 1: 2, 3: 6}),
                                    (Pair, 3, {1: 3, 2: 3, 3: 6})):
        plan = cls.__new__(cls)
        plan.device, plan.frames_out = torch.device("cpu"), frames_out
        plan._frames((4, 6, torch.uint8))
        for n, n_out in counts.items():
            assert tuple(plan._check_out(n, None).shape) == (n_out, 4, 6, 3)
            with pytest.raises(ValueError, match="out must be"):
                plan._check_out(n, torch.empty((n_out + 1, 4, 6, 3), dtype=torch.uint8))


# what include/crtfx_interlace.h states for the twelve builds: VGPRs as built
HEADER_VGPRS = {
    "k_interlace<none,u8,vec>": 12, "k_interlace<none,f16,vec>": 18, "k_interlace<linear,u8,vec>": 28, "k_interlace<linear,f16,vec>": 44,
    "k_interlace<complex,u8,vec>": 43, "k_interlace<complex,f16,vec>": 57,
    "k_interlace<none,u8,general>": 5, "k_interlace<none,f16,general>": 5, "k_interlace<linear,u8,general>": 11, "k_interlace<linear,f16,general>": 12,
    "k_interlace<complex,u8,general>": 20, "k_interlace<complex,f16,general>": 22}


def test_interlace_kernels_have_no_scratch_and_the_headers_registers():
    """Registers, LDS and scratch of the twelve builds, read from the built library's code objects (tools/kernel_resources.py): no LDS, no
    scratch memory, no spills, no AGPRs — and the figures the header quotes are the figures of this build."""
    import kernel_resources
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    res = kernel_resources.resources(_lib.LIB_PATH)
    found = {n.replace("crtfx_interlace_impl::", "").replace("crtfx_deint_impl::", "").replace(", ", ","): v
             for n, v in res.items() if n.startswith("crtfx_interlace_impl::")}
    assert set(found) == set(HEADER_VGPRS), sorted(found)
    hdr = open(HEADER).read()
    for name, v in found.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["group_segment_fixed_size"] == 0 and v["agpr_count"] == 0, (name, v)
        assert v["vgpr_count"] == HEADER_VGPRS[name], (name, v["vgpr_count"])
        assert re.search(rf"{re.escape(name)} {HEADER_VGPRS[name]}\b", hdr), name
    assert "no AGPRs, no LDS, no scratch, no spills" in hdr
    assert len([n for n in res if n.startswith("crtfx_deint_impl::")]) == 16   # the deinterlacer's builds are its own still


# ---- process_frames and the CLI: every refusal comes before a device --------------------------------------------------------------------------

def _refusing_process_frames(monkeypatch):
    import torch
    import pythoncrt_amd as pc

    def never():
        raise AssertionError("a frame was read")
        yield

    def no_device():
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    return lambda h=46, **kw: pc.process_frames(never(), lambda a: None, 80, h, 30.0, 1, **kw)


def test_process_frames_refusals(monkeypatch):
    run = _refusing_process_frames(monkeypatch)
    for bad in ("on", "", None, "TFF", True, 1, "none"):
        with pytest.raises(ValueError, match="deliver_interlace must be"):
            run(deliver_interlace=bad)
    for bad in ("vlpf", "", None, "LINEAR", 0, "off"):
        for order in ("off", "tff"):
            with pytest.raises(ValueError, match="deliver_lowpass must be"):
                run(deliver_interlace=order, deliver_lowpass=bad)
    for lowpass in ("linear", "complex"):
        for kw in (dict(), dict(deliver_interlace="off")):
            with pytest.raises(ValueError, match="nothing to filter"):
                run(deliver_lowpass=lowpass, **kw)
    for order in model.ORDERS:
        with pytest.raises(ValueError, match="no two fields"):                  # a render of one row delivered as rendered
            run(h=1, deliver_interlace=order)
        with pytest.raises(ValueError, match="no two fields"):
            run(deliver_interlace=order, deliver_size=(1, 80))
        with pytest.raises(ValueError, match="no two fields"):
            run(deliver_interlace=order, deliver_size=(1, 40), deliver_fit="pad", out_pix_fmt="uyvy422")
    # what is admitted: the next thing asked for is the device
    for kw in (dict(deliver_interlace="tff"), dict(deliver_interlace="bff", deliver_lowpass="complex"), dict(deliver_interlace="off", deliver_lowpass="none"),
               dict(deliver_interlace="tff", deliver_lowpass="linear", deinterlace="edge", deinterlace_fields="both"),
               dict(deliver_interlace="bff", chain_pix="half", dither="ordered", deliver_size=(2, 80)),
               dict(h=1, deliver_interlace="tff", deliver_size=(2, 80)),
               dict(deliver_interlace="tff", in_pix_fmt="p010le", out_pix_fmt="yuv444p10le", deliver_lowpass="complex"), dict()):
        with pytest.raises(AssertionError, match="the device was asked for"):
            run(**kw)


def test_cli_refusals_and_the_sharded_cli(tmp_path, monkeypatch):
    from pythoncrt_amd import cli
    src = tmp_path / "in.rgb"
    src.write_bytes(bytes(46 * 80 * 3))
    out = tmp_path / "out.rgb"
    base = ["--input", str(src), "--output", str(out), "--width", "80", "--height", "46"]

    def refused(extra, *words, args=base):
        with pytest.raises(SystemExit) as e:
            cli.main(args + extra)
        assert e.value.code not in (0, None) and all(w in str(e.value) for w in words), (extra, str(e.value))
        assert not out.exists()
    refused(["--deliver-lowpass", "linear"], "--deliver-lowpass linear", "--deliver-interlace", "nothing to filter")
    refused(["--deliver-interlace", "off", "--deliver-lowpass", "complex"], "--deliver-lowpass complex", "nothing to filter")
    one_row = ["--input", str(src), "--output", str(out), "--width", "80", "--height", "1"]
    for order in model.ORDERS:
        refused(["--deliver-interlace", order], "--deliver-interlace " + order, "no two fields", args=one_row)
        refused(["--deliver-interlace", order, "--deliver-width", "80", "--deliver-height", "1"], "--deliver-interlace " + order, "no two fields")
    for extra in (["--deliver-interlace", "on"], ["--deliver-lowpass", "vlpf"], ["--deliver-interlace"], ["--deliver-lowpass"]):
        with pytest.raises(SystemExit):                                         # argparse's own refusal of an unknown choice
            cli.main(base + extra)
    assert not any(act.dest in ("deliver_interlace", "deliver_lowpass") for act in cli.build_parser()._actions)
    assert not any(act.dest in ("deliver_interlace", "deliver_lowpass") for act in cli.add_input_flags(cli.build_parser())._actions)
    assert sum(act.dest in ("deliver_interlace", "deliver_lowpass") for act in cli.add_output_flags(cli.build_parser())._actions) == 2
    parse = cli.add_input_flags(cli.add_output_flags(cli.build_parser())).parse_args
    a = parse(base)
    spec, ranks = cli.check_flags(a)
    assert (a.deliver_interlace, a.deliver_lowpass) == ("off", "none") and spec.weave is None
    assert spec.deliver is None and spec.half is False and ranks is None
    a = parse(base + ["--deliver-interlace", "bff", "--deliver-lowpass", "complex"])
    spec, ranks = cli.check_flags(a)
    assert spec.weave == ("bff", "complex") and spec.deliver is None and spec.half is False and ranks is None
    a = parse(one_row + ["--deliver-interlace", "tff", "--deliver-width", "80", "--deliver-height", "2"])
    spec, ranks = cli.check_flags(a)
    assert spec.weave == ("tff", "none")
    assert "--deliver-interlace bff --deliver-lowpass linear" in cli.__doc__ and "+ilme+ildct" in cli.__doc__
    monkeypatch.setenv("CRTFX_FORCE_DIST", "1")
    refused(["--deliver-interlace", "tff"], "--deliver-interlace / --deliver-lowpass is not supported by the sharded CLI")
    refused(["--deliver-interlace", "bff", "--deliver-lowpass", "linear"], "--deliver-interlace / --deliver-lowpass is not supported by the sharded CLI")
    refused(["--deliver-lowpass", "linear"], "nothing to filter")


def test_open_output_plans_delivered_frames(tmp_path):
    """A regular input of 11 chain frames in batches of 4 under --deliver-interlace: batches of 2, 2 and ceil(3 / 2) delivered frames, at
    offsets of delivered frames, and the file sized to their sum under --io mapped; without `frames` the plan of before."""
    from pythoncrt_amd import cli
    src = tmp_path / "in.raw"
    src.write_bytes(bytes(11 * 10))
    parse = cli.add_input_flags(cli.add_output_flags(cli.build_parser())).parse_args
    for io in ("staged", "mapped"):
        a = parse(["--input", str(src), "--output", str(tmp_path / f"out_{io}.raw"), "--width", "1", "--height", "1", "--io", io])
        with open(src, "rb", buffering=0) as fin:
            fout, in_pos, out_pos, _, plan = cli.open_output(a, fin, a.output, 4, 10, 7, 1, lambda m: -(-m // 2))
            assert in_pos and out_pos and plan == [(0, 14), (14, 14), (28, 14)]
            assert os.fstat(fout.fileno()).st_size == (42 if io == "mapped" else 0)
            fout.close()
            fout, _, _, _, plan = cli.open_output(a, fin, a.output, 4, 10, 7, 1)
            assert plan == [(0, 28), (28, 28), (56, 21)] and os.fstat(fout.fileno()).st_size == (77 if io == "mapped" else 0)
            fout.close()
            fout, _, _, _, plan = cli.open_output(a, fin, a.output, 4, 10, 7, 2, lambda m: -(-m // 2))       # both fields in front: 22 chain frames
            assert plan == [(k * 14, 14) for k in range(5)] + [(70, 7)]
            fout.close()


# ---- which stages DeliveryEnd builds, and the counts it returns ---------------------------------------------------------------------------------

RESIZES = (ingest.IngestResize, resize16.ResizeHalf, resample.Resample)


@pytest.fixture
def built(monkeypatch):
    """Canvas, the resize plans, Narrow, Lut3D and Interlace record (class, positional arguments, keywords) instead of creating a plan."""
    log = []
    for cls in RESIZES + (canvas.Canvas, depth.Narrow, lut3d.Lut3D, interlace.Interlace):
        def init(self, *args, _cls=cls, **kw):
            log.append((_cls, args, kw))
        monkeypatch.setattr(cls, "__init__", init)
    return log


class _Egress:
    frame_bytes = 123


def _end(monkeypatch, out_pix_fmt="rgb24", **kw):
    monkeypatch.setattr(formats, "egress_plan", lambda *a: None if a[2] == "rgb24" else _Egress())
    a = dict(deliver=None, deliver_filter="bilinear")
    a.update(kw)
    deliver, flt = a.pop("deliver"), a.pop("deliver_filter")
    return ends.DeliveryEnd("dev", (24, 32), a.pop("pix"), out_pix_fmt, "bt601", "tv", "center", deliver, flt, **a)


def test_delivery_end_stages(built, monkeypatch):
    import torch
    u8, f16 = torch.uint8, torch.float16
    R, D = (24, 32), (48, 96)
    # without the keyword, and with None: what was built before, and the counts of before
    for kw in (dict(), dict(interlace=None)):
        del built[:]
        end = _end(monkeypatch, pix=u8, **kw)
        assert built == [] and end.stages == [] and end.interlace is None
        assert [end.frames(m) for m in (0, 1, 2, 5, 8)] == [0, 1, 2, 5, 8] and end.shape(4) == (4,) + R + (3,)
        end = _end(monkeypatch, "nv12", pix=f16, deliver=D, deliver_fit="pad", narrow="ordered", **kw)
        assert [b[0] for b in built] == [resize16.ResizeHalf, canvas.Canvas, depth.Narrow] and end.interlace is None and end.frames(5) == 5
    # as rendered: the Interlace is the only stage, at the render size and on the chain's pixel type
    for pix, weave in ((u8, ("tff", "none")), (f16, ("bff", "complex"))):
        del built[:]
        end = _end(monkeypatch, pix=pix, interlace=weave)
        assert built == [(interlace.Interlace, ("dev", R), {"order": weave[0], "lowpass": weave[1], "dtype": pix})]
        assert [hw for _, hw in end.stages] == [R] and end.stages[0][0] is end.interlace
        assert [end.frames(m) for m in (0, 1, 2, 5, 8)] == [0, 1, 1, 3, 4] and end.frame_bytes == 24 * 32 * 3
    # a padded delivery on a half chain with a LUT and a dither: LUT, resize, Canvas, INTERLACE at the delivery size on half, Narrow, egress
    del built[:]
    end = _end(monkeypatch, "uyvy422", pix=f16, deliver=D, deliver_fit="pad", narrow="ordered", lut="cube", interlace=("bff", "linear"))
    assert [b[0] for b in built] == [lut3d.Lut3D, resize16.ResizeHalf, canvas.Canvas, interlace.Interlace, depth.Narrow]
    assert built[3] == (interlace.Interlace, ("dev", D), {"order": "bff", "lowpass": "linear", "dtype": f16})
    assert [type(st) for st, _ in end.stages] == [lut3d.Lut3D, resize16.ResizeHalf, canvas.Canvas, interlace.Interlace, depth.Narrow]
    assert [hw for _, hw in end.stages] == [R, (48, 64), D, D, D] and end.frame_bytes == 123 and end.shape(3) == (3, 123)
    # a cropped delivery: Canvas, resize, Interlace; a stretched one with a filter: Resample, Interlace
    del built[:]
    end = _end(monkeypatch, pix=u8, deliver=D, deliver_fit="crop", interlace=("tff", "linear"))
    assert [b[0] for b in built] == [canvas.Canvas, ingest.IngestResize, interlace.Interlace] and built[2][1] == ("dev", D) and built[2][2]["dtype"] == u8
    del built[:]
    end = _end(monkeypatch, pix=u8, deliver=D, deliver_filter="lanczos", interlace=("tff", "none"))
    assert [b[0] for b in built] == [resample.Resample, interlace.Interlace] and built[1][1] == ("dev", D)


def test_delivery_end_buffers_and_counts_behind_the_interlace(built, monkeypatch):
    """slots(): a stage in front of the Interlace writes B frames, the Interlace and every stage behind it, the egress plan's output included,
    ceil(B / 2); run(d, m) hands each stage the frames of the one in front and returns ceil(m / 2) frames."""
    import torch
    shapes = []
    real_empty = torch.empty

    def empty(shape, dtype=None, device=None):
        shapes.append((tuple(shape), dtype, device))
        return real_empty(shape, dtype=dtype)                                   # on the host: the shapes are what is checked
    monkeypatch.setattr(torch, "empty", empty)
    u8, f16 = torch.uint8, torch.float16
    D = (48, 96)
    end = _end(monkeypatch, "uyvy422", pix=f16, deliver=D, deliver_fit="pad", narrow="none", interlace=("tff", "linear"))
    _Egress.run = lambda self, x, out: calls.append((_Egress, tuple(x.shape), tuple(out.shape))) or out
    dev_out = [real_empty((6, 24, 32, 3), dtype=f16) for _ in range(2)]
    fin, send = end.slots(dev_out)
    assert [s for s in shapes if s[2] == "dev"] == ([((6, 48, 64, 3), f16, "dev")] * 2 + [((6,) + D + (3,), f16, "dev")] * 2 +
                                                   [((3,) + D + (3,), f16, "dev")] * 2 + [((3,) + D + (3,), u8, "dev")] * 2 + [((3, 123), u8, "dev")] * 2)
    assert fin is end.bufs[-1] and tuple(send[0].shape) == end.shape(end.frames(6)) == (3, 123)
    calls = []
    for st, _ in end.stages:
        st.run = lambda x, out, _st=st: calls.append((type(_st), tuple(x.shape), tuple(out.shape))) or out
    for m, md in ((6, 3), (5, 3), (2, 1), (1, 1)):
        del calls[:]
        got = end.run(1, m)
        assert tuple(got.shape) == (md, 123) and got.data_ptr() == send[1].data_ptr()
        assert calls == [(resize16.ResizeHalf, (m, 24, 32, 3), (m, 48, 64, 3)), (canvas.Canvas, (m, 48, 64, 3), (m,) + D + (3,)),
                         (interlace.Interlace, (m,) + D + (3,), (md,) + D + (3,)), (depth.Narrow, (md,) + D + (3,), (md,) + D + (3,)),
                         (_Egress, (md,) + D + (3,), (md, 123))]
    # rgb24 as rendered: the Interlace's buffer is what is downloaded
    del shapes[:]
    end = _end(monkeypatch, pix=u8, interlace=("bff", "none"))
    dev_out = [real_empty((4, 24, 32, 3), dtype=u8) for _ in range(2)]
    fin, send = end.slots(dev_out)
    assert fin is send and tuple(send[0].shape) == (2, 24, 32, 3) == end.shape(end.frames(4))
    end.stages[0][0].run = lambda x, out: out
    assert tuple(end.run(0, 3).shape) == (2, 24, 32, 3) and tuple(end.run(0, 4).shape) == (2, 24, 32, 3)
    # and without the keyword: every buffer and the return value count the chain's frames
    end = _end(monkeypatch, pix=u8)
    fin, send = end.slots(dev_out)
    assert fin is dev_out and send is dev_out and tuple(end.run(0, 3).shape) == (3, 24, 32, 3)
