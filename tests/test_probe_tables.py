"""The source probe without a GPU (include/crtfx_probe.h): the model against a per-pixel restatement of the header and against what follows
from the rule (constants, ramps, the histogram total, float64 sums, every half pattern, the 64-bit bounds, h = 1, 2, 3), the field-rate scenes
classified with the stated margin, letterboxed and pillarboxed frames giving the exact window, the C-ABI bound symbol for symbol and
refusing bad arguments before it touches a device, probe_frames and the command-line module refusing with the device never asked for, and
the builds' registers and LDS against the header."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pythoncrt_amd import _lib, _stage, probe  # noqa: E402
from tests import deint_model as dm  # noqa: E402
from tests import probe_model as model  # noqa: E402

HEADER = os.path.join(ROOT, "include", "crtfx_probe.h")
DTYPES = (np.uint8, np.float16)
MARGIN = 1.5                            # what every classified scene keeps to probe.RATIO, on either side of it


# ---- the arithmetic -------------------------------------------------------------------------------------------------------------------------

def _q(bits16):
    """The header's quantiser of one half pattern, in Python floats."""
    f = float(np.uint16(bits16).view(np.float16))
    if f != f:
        return 0
    t = min(max(4.0 * f, 0.0), 1020.0)
    lo = int(t // 1)
    frac = t - lo
    return lo + (1 if frac > 0.5 or (frac == 0.5 and lo % 2 == 1) else 0)


def _loop_record(frame, prev):
    """One record, pixel by pixel, as the header states it."""
    h, w = frame.shape[:2]

    def code(a, y, x, k):
        return 4 * int(a[y, x, k]) if a.dtype == np.uint8 else _q(a.view(np.uint16)[y, x, k])

    def Y(a, y, x):
        return (54 * code(a, y, x, 0) + 183 * code(a, y, x, 1) + 19 * code(a, y, x, 2) + 128) >> 8
    rec = [0] * model.words(h, w)
    rec[0] = 0 if prev is None else 1
    rec[1:4], rec[4:7] = [1 << 40] * 3, [0] * 3
    sums = {8: 0, 10: 0, 12: 0, 14: 0}
    for y in range(h):
        for x in range(w):
            for k in range(3):
                rec[1 + k], rec[4 + k] = min(rec[1 + k], code(frame, y, x, k)), max(rec[4 + k], code(frame, y, x, k))
            v = Y(frame, y, x)
            sums[8] += v
            rec[16 + (v >> 2)] += 1
            rec[272 + y] += v
            rec[272 + h + x] += v
            if 1 <= y <= h - 2:
                comb = Y(frame, y - 1, x) + Y(frame, y + 1, x)
                sums[10] += abs(comb - 2 * v)
                if prev is not None:
                    sums[12 if y % 2 == 0 else 14] += abs(comb - 2 * Y(prev, y, x))
    for at, v in sums.items():
        rec[at], rec[at + 1] = v & 0xffffffff, v >> 32
    return np.array(rec, dtype=np.uint32)


def _frames(n, h, w, dtype, seed):
    f = dm.noise(h, w, n, dtype, seed)
    if dtype == np.float16:                                                    # patterns that cross every rule of the quantiser
        f = f.copy()
        flat = f.reshape(-1)
        flat[::7] = np.resize(np.array([np.nan, np.inf, -np.inf, -0.0, 255.5, 254.875, 0.125, 0.375, 6e-8, 65504.0, 100.1, -3.0], dtype=np.float16), flat[::7].size)
    return f


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", [(1, 1), (1, 5), (2, 3), (3, 4), (4, 7), (7, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_model_is_the_headers_rule_pixel_by_pixel(size, dtype):
    f = _frames(3, size[0], size[1], dtype, seed=size[0] * 10 + size[1])
    for prev in (None, f[2]):
        got = model.records(f[:2], prev)
        for i in range(2):
            assert np.array_equal(got[i], _loop_record(f[i], prev if i == 0 else f[i - 1])), (size, i, prev is None)
    assert model.records(f[:0]).shape == (0, model.words(*size))


def test_every_half_pattern_through_the_quantiser():
    pats = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    q = model.codes(pats.view(np.float16))
    assert q.min() == 0 and q.max() == 1020 and np.array_equal(q, [_q(p) for p in pats])
    nan = np.isnan(pats.view(np.float16))
    assert nan.sum() == 2046 and not q[nan].any() and not q[pats >= 0x8000].any()
    assert np.array_equal(model.codes(np.arange(256, dtype=np.uint8)), 4 * np.arange(256))
    # ... and a frame that holds them all: the histogram counts each luma once
    frame = np.resize(pats, (64, 342, 3)).view(np.float16)
    rec = model.record(frame)
    assert int(rec[16:272].sum()) == 64 * 342 and np.array_equal(rec[16:272], np.bincount(model.luma(frame).reshape(-1) >> 2, minlength=256))


@pytest.mark.parametrize("dtype", DTYPES)
def test_constants_ramps_and_float_sums(dtype):
    h, w = 9, 14
    for u in (0, 1, 37, 255):
        f = np.full((1, h, w, 3), u, dtype=dtype)
        r = probe.decode(model.records(f, f[0]), (h, w))[0]
        assert r.rgb_min == r.rgb_max == (4 * u,) * 3 and r.sum_y == 4 * u * h * w and (r.s_cur, r.s_even, r.s_odd) == (0, 0, 0) and r.had_prev
        assert int(r.hist[u]) == h * w == int(r.hist.sum()) and (r.rows == 4 * u * w).all() and (r.cols == 4 * u * h).all()
    ramp = np.broadcast_to((10 * np.arange(h))[:, None, None], (h, w, 3)).astype(dtype)[None]      # linear down the rows: no comb
    r = probe.decode(model.records(ramp), (h, w))[0]
    assert r.s_cur == 0 and not r.had_prev and (r.s_even, r.s_odd) == (0, 0) and list(r.rows) == [40 * y * w for y in range(h)]
    f = _frames(2, 23, 40, dtype, seed=4)
    Y = model.luma(f).astype(np.float64)
    r = probe.decode(model.records(f), (23, 40))[1]
    assert r.sum_y == Y[1].sum() and np.array_equal(r.rows, Y[1].sum(axis=1)) and np.array_equal(r.cols, Y[1].sum(axis=0))
    assert r.s_cur == np.abs(Y[1, :-2] + Y[1, 2:] - 2 * Y[1, 1:-1]).sum()
    comb = np.abs(Y[1, :-2] + Y[1, 2:] - 2 * Y[0, 1:-1]).sum(axis=1)
    assert (r.s_even, r.s_odd) == (comb[1::2].sum(), comb[0::2].sum())         # comb[j] is row j + 1
    assert int(r.hist.sum()) == 23 * 40 and 0 <= Y.min() and Y.max() <= 1020
    white = np.full((1, 2, 2, 3), 255, dtype=dtype)
    assert probe.decode(model.records(white), (2, 2))[0].sum_y == 4 * 1020      # the weights sum to 256: white is 1020


def test_small_heights_and_the_64_bit_bounds():
    for h in (1, 2, 3):
        f = _frames(2, h, 6, np.uint8, seed=h)
        r = probe.decode(model.records(f), (h, 6))[1]
        assert r.had_prev and ((r.s_cur, r.s_even, r.s_odd) == (0, 0, 0)) == (h < 3)
        assert r.s_even == 0                                                  # h = 3: row 1 is the only interior row, and it is odd
    side, top = 32767, 1020
    assert side * top < 1 << 32 and side * side < 1 << 32                      # a row or column sum, a histogram bin
    assert 1 << 32 <= side * side * top < 1 << 41 and side * side * 2 * top < 1 << 42      # the sum of Y, an S sum: 64 bits
    assert 8 * 8 * 2 * top < 1 << 18 and 256 * 8 * 8 * 2 * top < 1 << 26       # a lane's partial sums, a block's (crtfx_probe.h)
    lib = _lib.load()
    for h, w in ((1, 1), (1, 2), (2, 8), (480, 720), (1080, 1920), (32767, 32767), (5, 6)):
        got = lib.crtfx_probe_words(h, w)
        assert got == model.words(h, w) == probe.words(h, w) and got % 2 == 0 and 272 + h + w <= got <= 273 + h + w
    assert [lib.crtfx_probe_words(h, w) for h, w in ((0, 4), (4, 0), (32768, 4), (4, 32768), (-1, -1))] == [0] * 5


# ---- the field order and the window ---------------------------------------------------------------------------------------------------------

SCENES = [((24, 40), None, None), ((46, 80), None, None), ((160, 32), (176, 48), (8, 8)), ((48, 40), (48, 64), (0, 12))]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size,full,at", SCENES, ids=lambda v: "x".join(map(str, v)) if v else "bare")
def test_field_rate_scenes_are_classified_with_the_stated_margin(size, full, at, dtype):
    """Woven TFF / BFF, progressive and still scenes (tests/probe_model.scene: stripes that move one pixel per field), bare and inside bars
    that hold noise: five frame pairs.  Every classified scene keeps a factor of MARGIN to the default ratio, on its side of it."""
    assert 1.01 * MARGIN <= probe.RATIO <= 2.2 * 1.1 / MARGIN
    for kind in model.KINDS:
        f = model.scene(kind, 6, size[0], size[1], dtype)
        if full:
            f = model.boxed(f, full, at)
        hw = full or size
        rep = probe.ProbeReport(hw).add(model.records(f[:2])).add(model.records(f[2:], f[1]))      # in two batches
        assert rep.frames == 6 and rep.pairs == 5
        assert (rep.s_cur, rep.s_even, rep.s_odd) == model.sums(model.records(f))
        e, o = rep.s_even, rep.s_odd
        if kind in ("tff", "bff"):
            big, small = (e, o) if kind == "tff" else (o, e)
            assert big >= MARGIN * probe.RATIO * small, (kind, e, o)
            assert rep.field_order() == kind and rep.suggest()["field_order"] == kind and rep.suggest()["deinterlace"] == "adaptive"
        elif e == 0 and o == 0:
            assert kind == "still" and not full and rep.field_order() is None and "deinterlace" not in rep.suggest()
        else:
            assert MARGIN * max(e, o) <= probe.RATIO * min(e, o), (kind, e, o)
            assert rep.field_order() == "progressive" and "deinterlace" not in rep.suggest()
    assert probe.ProbeReport((4, 4)).field_order() is None and probe.ProbeReport((4, 4)).add(model.records(f[:1, :4, :4])).field_order() is None
    tff = probe.ProbeReport(size).add(model.records(model.scene("tff", 6, size[0], size[1], dtype)))
    assert tff.field_order(ratio=3.5) == "progressive" and tff.field_order(ratio=1.0) == "tff"


@pytest.mark.parametrize("dtype", DTYPES)
def test_letterboxed_and_pillarboxed_frames_give_the_exact_window(dtype):
    pic = model.scene("progressive", 3, 30, 44, dtype)
    for full, at in (((48, 44), (9, 0)), ((30, 64), (0, 11)), ((50, 70), (7, 13))):      # letterboxed, pillarboxed, both: odd origins
        f = model.boxed(pic, full, at, noise=5)
        assert model.luma(f[:, :at[0]]).max(initial=0) < probe.LIMIT and model.luma(f[:, :, :at[1]]).max(initial=0) < probe.LIMIT      # the bars' noise lies below the limit
        rep = probe.ProbeReport(full).add(model.records(f))
        y, x = at
        assert rep.crop(round=1) == (y, x, 30, 44)
        y2, x2, ye, xe = -(-y // 2) * 2, -(-x // 2) * 2, (y + 30) // 2 * 2, (x + 44) // 2 * 2
        assert rep.crop() == rep.crop(round=2) == (y2, x2, ye - y2, xe - x2) and rep.suggest()["in_crop"] == rep.crop()
        y16, x16, ye16, xe16 = -(-y // 16) * 16, -(-x // 16) * 16, (y + 30) // 16 * 16, (x + 44) // 16 * 16
        assert rep.crop(round=16) == (y16, x16, ye16 - y16, xe16 - x16) and ye16 > y16 and xe16 > x16
        assert rep.crop(limit=1020) is None                                    # no row qualifies
        fl = rep.flags()
        assert fl[:8] == ["--in-crop-x", str(x2), "--in-crop-y", str(y2), "--in-crop-width", str(xe - x2), "--in-crop-height", str(ye - y2)]
    whole = probe.ProbeReport((30, 44)).add(model.records(pic))
    assert whole.crop() is None and whole.crop(round=1) is None and whole.suggest() == {} and whole.flags() == []      # the whole frame
    black = probe.ProbeReport((30, 44)).add(model.records(np.zeros_like(pic)))
    assert black.crop() is None and black.levels()["black_share"] == 1.0 and black.levels()["luma_max"] == 0
    lv = whole.levels()
    Y = model.luma(pic) >> 2
    assert (lv["luma_min"], lv["luma_max"]) == (Y.min(), Y.max()) and lv["luma_low"] <= lv["luma_high"] and abs(lv["luma_mean"] - model.luma(pic).mean() / 4) < 1e-9
    assert lv["r_max"] == model.codes(pic)[..., 0].max() / 4 and lv["white_share"] == (Y == 255).mean()
    assert json.loads(json.dumps(whole.as_dict())) == whole.as_dict()
    with pytest.raises(ValueError, match="words"):
        probe.decode(model.records(pic), (30, 46))


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------------------

_vp = ctypes.c_void_p
SIGNATURES = {
    "crtfx_probe_create": (ctypes.c_int, [ctypes.c_int] * 4 + [ctypes.POINTER(_vp)]),
    "crtfx_probe_destroy": (ctypes.c_int, [_vp]),
    "crtfx_probe_last_error": (ctypes.c_char_p, [_vp]),
    "crtfx_probe_run": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_int, _vp]),
    "crtfx_probe_set_option": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "crtfx_probe_last_plan": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_size_t]),
    "crtfx_probe_words": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
}


def test_symbols_are_bound_and_the_header_declares_them():
    assert _lib.PROBE_SYMBOLS == SIGNATURES and list(_lib.PROBE_SYMBOLS) == list(SIGNATURES) and _lib.PROBE_OPT_FORCE_GENERAL == 1
    assert _lib.PROBE_SYMBOLS == _lib.frame_symbols("probe", [ctypes.c_int] * 3, run=SIGNATURES["crtfx_probe_run"], words=SIGNATURES["crtfx_probe_words"])
    assert SIGNATURES["crtfx_probe_run"] == _lib.ADEINT_SYMBOLS["crtfx_adeint_run"]                # the previous frame first, as adeint's
    lib = _lib.load()
    for name, (res, args) in SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res, name
    hdr = open(HEADER).read()
    for text in ("CRTFX_PROBE_OPT_FORCE_GENERAL = 1", "NOT claimed is equality with any other filter", "(54 r + 183 g + 19 b + 128) >> 8",
                 "probe=k_probe<u8,vec>;frames=5", "272 + h + w", "bounded by its tile, not by its content"):
        assert text in hdr, text
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(crtfx_probe_\w+)\s*\(([^)]*)\)\s*;", hdr)}
    assert set(protos) == set(SIGNATURES) and len(protos) == 7, set(protos) ^ set(SIGNATURES)
    for name, args in protos.items():
        assert len(args.split(",")) == len(SIGNATURES[name][1]), name
    assert [a.split()[-1].lstrip("*") for a in protos["crtfx_probe_create"].split(",")] == ["device", "h", "w", "pix_fmt", "out_plan"]
    assert [a.split()[-1].lstrip("*") for a in protos["crtfx_probe_run"].split(",")] == [
        "plan", "prev_frame", "src_base", "src_stride_bytes", "records", "record_stride_bytes", "n", "stream"]
    others = set()
    for table in ("SYMBOLS", "INGEST_SYMBOLS", "EGRESS_SYMBOLS", "UNPACK_SYMBOLS", "DEEP_SYMBOLS", "YUV422_SYMBOLS", "DEEP444_SYMBOLS", "SITED_SYMBOLS",
                  "EGRESS_SITED_SYMBOLS", "RESIZE16_SYMBOLS", "RESAMPLE_SYMBOLS", "CANVAS_SYMBOLS", "DEPTH_SYMBOLS", "DEINT_SYMBOLS", "ADEINT_SYMBOLS",
                  "LUT3D_SYMBOLS", "INTERLACE_SYMBOLS", "SIGNAL_SYMBOLS"):
        others |= set(getattr(_lib, table))
    assert not set(SIGNATURES) & others
    names = {os.path.basename(s) for s in _lib.SOURCES}
    assert {"crtfx_probe.hip", "crtfx_probe.h", "crtfx_frame_host.h"} <= names and all(os.path.exists(s) for s in _lib.SOURCES)
    assert "crtfx_probe" in _lib.STAGE_UNITS
    import pythoncrt_amd as pc
    assert pc.Probe is probe.Probe and pc.ProbeReport is probe.ProbeReport and pc.probe_frames is probe.probe_frames
    assert {"Probe", "ProbeReport", "probe_frames"} <= set(pc.__all__)
    assert issubclass(pc.Probe, _stage.FramePlan) and pc.Probe._family == "probe" and pc.Probe._force_option == 1
    unit = open(os.path.join(_lib.CSRC, "crtfx_probe.hip")).read()
    assert "namespace crtfx_probe_impl" in unit and '#include "crtfx_frame_host.h"' in unit and "asm" not in unit
    assert (probe.W_HIST, probe.W_ROWS, probe.LIMIT) == (model.W_HIST, model.W_ROWS, 96)


GOOD = dict(device=0, h=9, w=24, pix_fmt=_lib.PIX_U8)


def _create(lib, no_out=False, **kw):
    a = dict(GOOD)
    a.update(kw)
    plan = ctypes.c_void_p(1)
    rc = lib.crtfx_probe_create(*(a[k] for k in GOOD), None if no_out else ctypes.byref(plan))
    return rc, plan, (lib.crtfx_probe_last_error(None) or b"").decode()


def test_create_refuses_bad_arguments_before_it_touches_a_device():
    lib = _lib.load()
    cases = [(dict(h=v), "h =") for v in (0, -3, 32768)] + [(dict(w=v), "w =") for v in (0, -3, 32768)] + [(dict(pix_fmt=v), "pix_fmt") for v in (2, -1, 7)]
    for kw, word in cases:
        rc, plan, msg = _create(lib, **kw)
        assert rc == _lib.E_INVALID and not plan.value and word in msg, (kw, rc, plan.value, msg)
    rc, plan, msg = _create(lib, no_out=True)
    assert rc == _lib.E_INVALID and "out_plan" in msg
    for kw in (dict(), dict(h=1, w=1), dict(h=1), dict(h=32767, w=32767, pix_fmt=_lib.PIX_F16)):      # h = 1 is allowed: the call gets as far as the device
        rc, plan, msg = _create(lib, device=4096, **kw)
        assert rc == _lib.E_HIP and not plan.value and msg == "no HIP device 4096", (kw, rc, msg)
    assert lib.crtfx_probe_destroy(None) == _lib.OK and lib.crtfx_probe_set_option(None, 1, 1) == _lib.E_INVALID
    assert lib.crtfx_probe_run(None, None, None, 0, None, 0, 1, None) == _lib.E_INVALID
    assert lib.crtfx_probe_last_plan(None, ctypes.create_string_buffer(8), 8) == _lib.E_INVALID


def test_python_plan_refuses_before_a_device():
    with pytest.raises(ValueError, match="ROCm device"):
        probe.Probe("cpu", (4, 4))
    with pytest.raises(TypeError):
        probe.Probe("cpu", (4, 4), order="tff")


# what include/crtfx_probe.h states for the four builds: (VGPRs, LDS bytes) as built
HEADER_RESOURCES = {"k_probe<u8,vec>": (90, 18592), "k_probe<f16,vec>": (90, 18592), "k_probe<u8,general>": (42, 16800), "k_probe<f16,general>": (44, 16800)}


def test_probe_kernels_have_no_scratch_and_the_headers_registers():
    import kernel_resources
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    res = kernel_resources.resources(_lib.LIB_PATH)
    found = {n.replace("crtfx_probe_impl::", "").replace("crtfx_deint_impl::", "").replace(", ", ","): v
             for n, v in res.items() if n.startswith("crtfx_probe_impl::")}
    init = found.pop("k_probe_init")
    assert init["group_segment_fixed_size"] == 0 and init["private_segment_fixed_size"] == 0
    assert set(found) == set(HEADER_RESOURCES), sorted(found)
    hdr = open(HEADER).read()
    for name, v in found.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["agpr_count"] == 0, (name, v)
        assert (v["vgpr_count"], v["group_segment_fixed_size"]) == HEADER_RESOURCES[name], (name, v["vgpr_count"], v["group_segment_fixed_size"])
        assert re.search(rf"{re.escape(name)} {HEADER_RESOURCES[name][0]} / {HEADER_RESOURCES[name][1]}\b", hdr), name
    assert "no AGPRs, no scratch, no spills" in hdr
    # the families whose device code the unit includes are untouched: exactly their kernels
    assert len([n for n in res if n.startswith("crtfx_deint_impl::")]) == 16 and len([n for n in res if n.startswith("crtfx_adeint_impl::")]) == 8


# ---- probe_frames and the command line: every refusal comes before a device -----------------------------------------------------------------

@pytest.fixture
def no_device(monkeypatch):
    import torch

    def asked():
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(torch.cuda, "is_available", asked)


def _never():
    raise AssertionError("a frame was read")
    yield


def test_probe_frames_refusals(no_device):
    import pythoncrt_amd as pc
    run = lambda **kw: pc.probe_frames(_never(), 80, 46, **kw)      # noqa: E731
    with pytest.raises(ValueError, match="in_pix_fmt must be 'rgb24'"):
        run(in_pix_fmt="yuv411p")
    for bad in ("Left", "", None):
        with pytest.raises(ValueError, match="in_chroma must be 'replicate', 'left' or 'center'"):
            run(in_pix_fmt="nv12", in_chroma=bad)
    for fmt in ("rgb24", "gbrp10le"):
        with pytest.raises(ValueError, match=f"in_chroma='left' with in_pix_fmt='{fmt}': only a 4:2:0 or 4:2:2 input"):
            run(in_pix_fmt=fmt, in_chroma="left")
    with pytest.raises(ValueError, match=r"in_size=\(40, 80\) differs from the output size \(46, 80\): a 10-bit input cannot be resized"):
        run(in_pix_fmt="p010le", in_size=(40, 80))
    with pytest.raises(ValueError, match="max_frames"):
        run(max_frames=-1)
    with pytest.raises(TypeError):
        run(deinterlace="edge")                                               # the probe measures that: no such keyword
    # the messages are process_frames' own
    for kw in (dict(in_pix_fmt="yuv411p"), dict(in_pix_fmt="rgb24", in_chroma="center"), dict(in_pix_fmt="p010le", out_pix_fmt="p010le", in_size=(40, 80))):
        with pytest.raises(ValueError) as a:
            pc.process_frames(_never(), lambda f: None, 80, 46, 30.0, 1, **kw)
        kw.pop("out_pix_fmt", None)
        with pytest.raises(ValueError) as b:
            run(**kw)
        assert str(a.value) == str(b.value)
    for kw in (dict(), dict(in_pix_fmt="nv12", in_size=(50, 90)), dict(in_pix_fmt="p010le"), dict(in_pix_fmt="uyvy422", in_chroma="left"), dict(in_pix_fmt="x2rgb10le")):
        with pytest.raises(AssertionError, match="the device was asked for"):
            run(**kw)


def test_the_command_line_module(no_device, tmp_path, capsys):
    from pythoncrt_amd import cli
    src = tmp_path / "in.rgb"
    src.write_bytes(bytes(46 * 80 * 3))
    base = ["--input", str(src), "--width", "80", "--height", "46"]

    def refused(extra, *words, args=base):
        with pytest.raises(SystemExit) as e:
            probe.main(args + extra)
        assert e.value.code not in (0, None) and all(w in str(e.value) or w in capsys.readouterr().err for w in words), (extra, str(e.value))
    refused(["--in-chroma", "left"], "--in-chroma left with --in-pix-fmt rgb24")
    refused(["--in-pix-fmt", "yuv411p"], "invalid choice")
    refused(["--in-matrix", "bt2020"], "invalid choice")
    refused(["--frames", "-2"], "--frames -2")
    refused([], "--width", args=["--input", str(src), "--width", "0", "--height", "46"])
    refused([], "required", args=["--width", "80", "--height", "46"])
    with pytest.raises(AssertionError, match="the device was asked for"):
        probe.main(base + ["--in-pix-fmt", "nv12", "--json"])
    # the four input flags are cli's own: the same choices and defaults
    ours = {a.option_strings[0]: a for a in probe.build_parser()._actions if a.option_strings}
    theirs = {a.option_strings[0]: a for a in cli.add_input_flags(cli.build_parser())._actions if a.option_strings}
    for flag in ("--in-pix-fmt", "--in-matrix", "--in-range", "--in-chroma"):
        assert ours[flag].choices == theirs[flag].choices and ours[flag].default == theirs[flag].default
    assert {"--input", "--width", "--height", "--frames", "--json"} <= set(ours) and "--in-crop-x" not in ours and "--output" not in ours
    # a report's flag line parses with cli's own parser
    rep = probe.ProbeReport((176, 48)).add(model.records(model.boxed(model.scene("bff", 4, 160, 32), (176, 48), (8, 8))))
    a = cli.add_input_flags(cli.add_output_flags(cli.build_parser())).parse_args(["--input", "x", "--output", "y", "--width", "48", "--height", "176"] + rep.flags())
    assert (a.in_crop_y, a.in_crop_x, a.in_crop_height, a.in_crop_width) == (8, 8, 160, 32) and (a.deinterlace, a.field_order) == ("adaptive", "bff")
    spec, ranks = cli.check_flags(a)
    assert spec.crop == (8, 8, 160, 32) and spec.deinterlace == ("adaptive", "bff", "first") and ranks is None
