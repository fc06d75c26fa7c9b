"""The geometry stage without a GPU (include/crtfx_canvas.h): the two fit rules against a literal table and their bounds, the numpy model
against hand-written frames, the C-ABI bound symbol for symbol and refusing bad arguments before it touches a device, the builds'
registers against the header, every refusal of process_frames(in_crop=, deliver_fit=, deliver_pad_color=) and of the CLI's flags, and —
with the plan classes replaced by recorders — which stages the two chain ends build."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pythoncrt_amd import _lib, _stage, canvas, ends, formats, ingest, resample, resize16  # noqa: E402
from tests import canvas_model as model  # noqa: E402

# (h, w), (dh, dw), fit_pad, fit_crop
FITS = [((1080, 1440), (1080, 1920), ((1080, 1440), (0, 240)), (135, 0, 810, 1440)),
        ((480, 640), (2160, 3840), ((2160, 2880), (0, 480)), (60, 0, 360, 640)),
        ((1080, 1920), (1080, 1440), ((810, 1440), (135, 0)), (0, 240, 1080, 1440)),
        ((2160, 3840), (480, 640), ((360, 640), (60, 0)), (0, 480, 2160, 2880)),
        ((18, 32), (9, 16), ((9, 16), (0, 0)), (0, 0, 18, 32)),
        ((7, 5), (9, 16), ((9, 6), (0, 5)), (2, 0, 3, 5)),
        ((5, 7), (16, 9), ((6, 9), (5, 0)), (0, 2, 5, 3)),
        ((1, 100), (50, 50), ((1, 50), (24, 0)), (0, 49, 1, 1)),
        ((6, 8), (9, 16), ((9, 12), (0, 2)), (0, 0, 5, 8)),
        ((13, 19), (5, 7), ((5, 7), (0, 0)), (0, 0, 13, 18)),
        ((1, 1), (3, 3), ((3, 3), (0, 0)), (0, 0, 1, 1))]


@pytest.mark.parametrize("size,deliver,pad,crop", FITS, ids=lambda v: str(v).replace(" ", ""))
def test_fit_table(size, deliver, pad, crop):
    for mod in (canvas, model):
        assert mod.fit_pad(size, deliver) == pad and mod.fit_crop(size, deliver) == crop, mod.__name__


def test_fit_results_stay_inside():
    """1 000 seeded size pairs in 1..4096: the inner frame fits the delivery and touches two of its sides, the window fits the frame and
    touches two of its sides, both are centred, and the product's functions are the model's."""
    rng = np.random.default_rng(20)
    for h, w, dh, dw in rng.integers(1, 4097, (1000, 4)).tolist():
        (ih, iw), (dy, dx) = canvas.fit_pad((h, w), (dh, dw))
        assert ((ih, iw), (dy, dx)) == model.fit_pad((h, w), (dh, dw))
        assert 1 <= ih <= dh and 1 <= iw <= dw and (ih == dh or iw == dw) and (dy, dx) == ((dh - ih) // 2, (dw - iw) // 2)
        assert dy + ih <= dh and dx + iw <= dw
        y, x, ch, cw = canvas.fit_crop((h, w), (dh, dw))
        assert (y, x, ch, cw) == model.fit_crop((h, w), (dh, dw))
        assert 1 <= ch <= h and 1 <= cw <= w and (ch == h or cw == w) and (y, x) == ((h - ch) // 2, (w - cw) // 2)
        assert y + ch <= h and x + cw <= w


def test_model_on_hand_written_frames():
    src = np.arange(36, dtype=np.uint8).reshape(3, 4, 3)                        # pixel (y, x) = [12 y + 3 x, + 1, + 2]
    F = [7, 200, 33]
    got = model.canvas(src, (3, 4), window=(1, 2, 2, 2), at=(0, 1), fill=F)       # crop and pad at once
    exp = np.array([[F, [18, 19, 20], [21, 22, 23], F],
                    [F, [30, 31, 32], [33, 34, 35], F],
                    [F, F, F, F]], dtype=np.uint8)
    assert got.dtype == np.uint8 and np.array_equal(got, exp)
    assert np.array_equal(model.canvas(src, (3, 4)), src)                       # the whole frame at (0, 0): identity
    assert np.array_equal(model.crop(src, (2, 0, 1, 3)), np.array([[[24, 25, 26], [27, 28, 29], [30, 31, 32]]], dtype=np.uint8))
    pad = model.canvas(src[:1, :2], (3, 4), at=(2, 2), fill=F)                  # a pure pad into the last corner
    exp = np.array([[F, F, F, F], [F, F, F, F], [F, F, [0, 1, 2], [3, 4, 5]]], dtype=np.uint8)
    assert np.array_equal(pad, exp)
    half = np.array([np.nan, -np.inf, -0.0], dtype=np.float16)
    out = model.canvas(np.broadcast_to(half, (2, 1, 1, 3)), (1, 2), at=(0, 1), fill=np.array([7, 200, 33], dtype=np.float16))
    assert out.shape == (2, 1, 2, 3) and np.array_equal(out[1, 0, 1].view(np.uint16), half.view(np.uint16))
    assert out[0, 0, 0].tolist() == [7.0, 200.0, 33.0]


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------------------

_vp = ctypes.c_void_p
SIGNATURES = {
    "crtfx_canvas_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint16),
                                           ctypes.POINTER(_vp)]),
    "crtfx_canvas_destroy": (ctypes.c_int, [_vp]),
    "crtfx_canvas_last_error": (ctypes.c_char_p, [_vp]),
    "crtfx_canvas_run": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_int, _vp]),
    "crtfx_canvas_set_option": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "crtfx_canvas_last_plan": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_size_t]),
}


def test_symbols_are_bound_and_the_header_declares_them():
    assert _lib.CANVAS_SYMBOLS == SIGNATURES and _lib.CANVAS_OPT_FORCE_GENERAL == 1
    lib = _lib.load()
    for name, (res, args) in SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res, name
    hdr = open(os.path.join(ROOT, "include", "crtfx_canvas.h")).read()
    assert "CRTFX_CANVAS_OPT_FORCE_GENERAL = 1" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(crtfx_canvas_\w+)\s*\(([^)]*)\)\s*;", hdr)}
    assert set(protos) == set(SIGNATURES) and len(protos) == 6, set(protos) ^ set(SIGNATURES)
    for name, args in protos.items():
        assert len(args.split(",")) == len(SIGNATURES[name][1]), name
    order = [a.split()[-1].split("[")[0].lstrip("*") for a in protos["crtfx_canvas_create"].split(",")]
    assert order == ["device", "pix_fmt", "src_h", "src_w", "win_y", "win_x", "win_h", "win_w", "dst_h", "dst_w", "dst_y", "dst_x", "fill", "out_plan"]
    others = set()
    for table in ("SYMBOLS", "INGEST_SYMBOLS", "EGRESS_SYMBOLS", "UNPACK_SYMBOLS", "DEEP_SYMBOLS", "YUV422_SYMBOLS", "DEEP444_SYMBOLS", "SITED_SYMBOLS",
                  "EGRESS_SITED_SYMBOLS", "RESIZE16_SYMBOLS", "RESAMPLE_SYMBOLS"):
        others |= set(getattr(_lib, table))
    assert not set(SIGNATURES) & others
    assert all(os.path.basename(f) in {os.path.basename(s) for s in _lib.SOURCES} for f in ("crtfx_canvas.hip", "crtfx_canvas.h"))
    assert all(os.path.exists(s) for s in _lib.SOURCES) and "crtfx_canvas" in _lib.STAGE_UNITS
    import pythoncrt_amd as pc
    assert pc.Canvas is canvas.Canvas and "Canvas" in pc.__all__ and issubclass(pc.Canvas, _stage.Handle)


GOOD = dict(device=0, pix_fmt=_lib.PIX_U8, src_h=13, src_w=19, win_y=3, win_x=4, win_h=5, win_w=7, dst_h=9, dst_w=16, dst_y=1, dst_x=2)


def _create(lib, fill=(7, 200, 33), null_fill=False, no_out=False, **kw):
    a = dict(GOOD)
    a.update(kw)
    plan = ctypes.c_void_p(1)
    rc = lib.crtfx_canvas_create(*(a[k] for k in GOOD), None if null_fill else (ctypes.c_uint16 * 3)(*fill), None if no_out else ctypes.byref(plan))
    return rc, plan, (lib.crtfx_canvas_last_error(None) or b"").decode()


def test_create_refuses_bad_arguments_before_it_touches_a_device():
    """Every refusal of crtfx_canvas_create comes before the device is asked for, so it holds on any machine; *out_plan is NULL and the
    message names the offending field."""
    lib = _lib.load()
    cases = [(dict(pix_fmt=7), "pixel format"), (dict(pix_fmt=-1), "pixel format"), (dict(null_fill=True), "fill")]
    cases += [({k: v}, k) for k in ("src_h", "src_w", "win_h", "win_w", "dst_h", "dst_w") for v in (0, -3, 32768)]
    cases += [(dict(win_y=-1), "win_y"), (dict(win_y=9), "win_y"), (dict(win_x=-1), "win_x"), (dict(win_x=13), "win_x"),      # 9 + 5 > 13, 13 + 7 > 19
              (dict(win_h=14, win_y=0, dst_h=20), "win_y"), (dict(win_w=20, win_x=0, dst_w=30), "win_x"),
              (dict(dst_y=-1), "dst_y"), (dict(dst_y=5), "dst_y"), (dict(dst_x=-1), "dst_x"), (dict(dst_x=10), "dst_x"),      # 5 + 5 > 9, 10 + 7 > 16
              (dict(dst_h=4), "dst_y"), (dict(dst_w=6), "dst_x"),
              (dict(fill=(0, 256, 0)), "fill[1]"), (dict(fill=(65535, 0, 0)), "fill[0]")]
    for kw, word in cases:
        rc, plan, msg = _create(lib, **kw)
        assert rc == _lib.E_INVALID and not plan.value and word in msg, (kw, rc, plan.value, msg)
    rc, plan, msg = _create(lib, no_out=True)
    assert rc == _lib.E_INVALID and "out_plan" in msg
    # what is admitted passes every check: the touching window and placement, and any half pattern as a fill.  What is left to fail
    # without a device is the device itself.
    import torch
    if not torch.cuda.is_available():
        for kw in (dict(), dict(win_y=8, win_x=12, dst_y=4, dst_x=9), dict(pix_fmt=_lib.PIX_F16, fill=(0x7e00, 0xfc00, 0x8000)),
                   dict(src_h=32767, src_w=32767, win_y=0, win_x=0, win_h=32767, win_w=32767, dst_h=32767, dst_w=32767, dst_y=0, dst_x=0)):
            rc, plan, msg = _create(lib, **kw)
            assert rc == _lib.E_HIP and not plan.value and "device" in msg.lower(), (kw, rc, msg)
    else:
        rc, plan, msg = _create(lib, device=4096)
        assert rc == _lib.E_HIP and not plan.value and "4096" in msg
    assert lib.crtfx_canvas_destroy(None) == _lib.OK and lib.crtfx_canvas_set_option(None, 1, 1) == _lib.E_INVALID
    assert lib.crtfx_canvas_run(None, None, 0, None, 0, 1, None) == _lib.E_INVALID
    assert lib.crtfx_canvas_last_plan(None, ctypes.create_string_buffer(8), 8) == _lib.E_INVALID


def test_python_plan_refuses_a_cpu_device():
    with pytest.raises(ValueError, match="ROCm device"):
        canvas.Canvas("cpu", (4, 4), (4, 4))


# what include/crtfx_canvas.h states for the four builds: VGPRs as built
HEADER_VGPRS = {"k_canvas<u8,vec>": 24, "k_canvas<f16,vec>": 24, "k_canvas<u8,general>": 4, "k_canvas<f16,general>": 4}


def test_canvas_kernels_hold_the_register_budget_and_the_header():
    """Registers, LDS and scratch of the four builds, read from the built library's code objects (tools/kernel_resources.py): at most 64
    VGPRs + AGPRs, no LDS, no scratch memory, no spills — and the figures the header quotes are the figures of this build."""
    import kernel_resources
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    res = kernel_resources.resources(_lib.LIB_PATH)
    found = {n.replace("crtfx_canvas_impl::", "").replace(", ", ","): v for n, v in res.items() if n.startswith("crtfx_canvas_impl::")}
    assert set(found) == set(HEADER_VGPRS), sorted(found)
    hdr = open(os.path.join(ROOT, "include", "crtfx_canvas.h")).read()
    for name, v in found.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["group_segment_fixed_size"] == 0 and v["vgpr_count"] + v["agpr_count"] <= 64 and v["agpr_count"] == 0, (name, v)
        assert v["vgpr_count"] == HEADER_VGPRS[name], (name, v["vgpr_count"])
        assert re.search(rf"{re.escape(name)} {HEADER_VGPRS[name]}\b", hdr), name
    assert "no AGPRs, no LDS, no scratch" in hdr


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
    return lambda **kw: pc.process_frames(never(), lambda a: None, 80, 46, 30.0, 1, **kw)


def test_process_frames_refusals(monkeypatch):
    run = _refusing_process_frames(monkeypatch)
    for bad in (5, (1, 2, 3), (1, 2, 3, 4, 5), "abcd", (0, 0, 10.5, 10), (0, 0, None, 10), (0, 0, True, 10),          # not four integers
                (0, 0, 0, 10), (0, 0, 10, 0), (0, 0, -4, 10), (-1, 0, 10, 10), (0, -1, 10, 10)):                      # a side < 1, an origin < 0
        for fmts in ({}, dict(in_pix_fmt="nv12"), dict(in_pix_fmt="p010le", out_pix_fmt="p010le")):
            with pytest.raises(ValueError, match="in_crop"):
                run(in_crop=bad, **fmts)
    for kw in (dict(in_crop=(0, 0, 47, 80)), dict(in_crop=(1, 0, 46, 80)), dict(in_crop=(0, 41, 46, 40)),               # leaves the render-size frame
               dict(in_crop=(0, 0, 21, 40), in_size=(20, 40)), dict(in_crop=(0, 1, 20, 40), in_size=(20, 40))):        # leaves in_size
        with pytest.raises(ValueError, match="in_crop.*leaves"):
            run(in_pix_fmt="nv12", **kw)
    with pytest.raises(ValueError, match="resize_on.*in_crop"):
        run(in_crop=(0, 0, 10, 10), resize_on="host")
    for bad in ("fill", "", None, "PAD"):
        with pytest.raises(ValueError, match="deliver_fit"):
            run(deliver_fit=bad, deliver_size=(23, 40))
    for fit in ("pad", "crop"):
        for kw in (dict(), dict(deliver_size=None), dict(deliver_size=(46, 80))):
            with pytest.raises(ValueError, match="deliver_fit.*nothing to fit"):
                run(deliver_fit=fit, **kw)
    for bad in ((0, 0, 256), (-1, 0, 0), (0, 0), (1, 2, 3, 4), "red", 7, (0.5, 0, 0), (None, 0, 0)):
        with pytest.raises(ValueError, match="deliver_pad_color"):
            run(deliver_pad_color=bad, deliver_fit="pad", deliver_size=(23, 40))
    # a 10-bit input: a window of the render size is allowed (so the refusal is not reached: the device is asked for), any other is "cannot be resized"
    ten = dict(in_pix_fmt="p010le", out_pix_fmt="p010le")
    with pytest.raises(ValueError, match="in_crop.*cannot be resized"):
        run(in_crop=(0, 0, 40, 80), **ten)
    with pytest.raises(ValueError, match="in_crop.*cannot be resized"):
        run(in_crop=(2, 2, 46, 78), in_size=(50, 90), **ten)
    with pytest.raises(AssertionError, match="the device was asked for"):
        run(in_crop=(2, 4, 46, 80), in_size=(50, 90), **ten)
    with pytest.raises(ValueError, match=r"in_size=\(50, 90\) differs from the output size \(46, 80\): a 10-bit input cannot be resized"):
        run(in_size=(50, 90), **ten)                                            # without in_crop: the refusal as it was


def test_cli_refusals_and_the_sharded_cli(tmp_path, monkeypatch):
    from pythoncrt_amd import cli
    src = tmp_path / "in.rgb"
    src.write_bytes(bytes(46 * 80 * 3))
    out = tmp_path / "out.rgb"
    base = ["--input", str(src), "--output", str(out), "--width", "80", "--height", "46"]
    deliver = ["--deliver-width", "40", "--deliver-height", "40"]

    def refused(extra, *words):
        with pytest.raises(SystemExit) as e:
            cli.main(base + extra)
        assert e.value.code not in (0, None) and all(w in str(e.value) for w in words), (extra, str(e.value))
        assert not out.exists()
    for extra in (["--in-crop-width", "40"], ["--in-crop-height", "20"], ["--in-crop-x", "3"], ["--in-crop-y", "3"],
                  ["--in-crop-x", "3", "--in-crop-y", "3", "--in-crop-width", "40"]):
        refused(extra, "--in-crop-width", "--in-crop-height", "go together")
    for extra in (["--in-crop-width", "81", "--in-crop-height", "46"], ["--in-crop-width", "80", "--in-crop-height", "46", "--in-crop-y", "1"],
                  ["--in-crop-width", "40", "--in-crop-height", "20", "--in-crop-x", "41"], ["--in-crop-width", "-4", "--in-crop-height", "20"],
                  ["--in-crop-width", "40", "--in-crop-height", "20", "--in-crop-x", "-1"]):
        refused(extra, "--in-crop-width", "leaves")
    refused(["--deliver-fit", "pad"], "--deliver-fit pad", "nothing to fit")
    refused(["--deliver-fit", "crop", "--deliver-width", "80", "--deliver-height", "46"], "--deliver-fit crop", "nothing to fit")
    for bad in ("0,0,256", "1,2", "-1,0,0", "red", "1,2,3,4", ""):
        refused(deliver + ["--deliver-fit", "pad", "--deliver-pad-color=" + bad], "--deliver-pad-color")
    refused(["--in-pix-fmt", "p010le", "--out-pix-fmt", "p010le", "--in-crop-width", "40", "--in-crop-height", "46"], "--in-crop-width", "cannot be resized")
    with pytest.raises(SystemExit):                                             # argparse's own refusal of an unknown choice
        cli.main(base + deliver + ["--deliver-fit", "fill"])
    parse = cli.add_input_flags(cli.add_output_flags(cli.build_parser())).parse_args
    a = parse(base)
    assert (a.in_crop_x, a.in_crop_y, a.in_crop_width, a.in_crop_height, a.deliver_fit, a.deliver_pad_color) == (0, 0, 0, 0, "stretch", "0,0,0")
    assert cli.in_crop_from_args(a) is None and cli.pad_color_from_args(a) == (0, 0, 0)
    a = parse(base + ["--in-crop-x", "4", "--in-crop-y", "6", "--in-crop-width", "64", "--in-crop-height", "36", "--deliver-pad-color", "7,200,33"])
    assert cli.in_crop_from_args(a) == (6, 4, 36, 64) and cli.pad_color_from_args(a) == (7, 200, 33)
    a = parse(base + ["--in-crop-width", "80", "--in-crop-height", "46"])
    assert cli.in_crop_from_args(a) == (0, 0, 46, 80)                           # the whole frame at (0, 0) is a window
    assert not any(act.dest.startswith(("in_crop", "deliver_fit", "deliver_pad")) for act in cli.build_parser()._actions)
    monkeypatch.setenv("CRTFX_FORCE_DIST", "1")
    for extra, flag in ((["--in-crop-width", "40", "--in-crop-height", "20"], "--in-crop-width"), (["--in-crop-x", "2"], "--in-crop-x"),
                        (["--deliver-fit", "pad"], "--deliver-fit"), (["--deliver-pad-color", "1,2,3"], "--deliver-pad-color")):
        refused(extra, "sharded CLI", flag)


# ---- which stages the chain ends build --------------------------------------------------------------------------------------------------------

RESIZES = (ingest.IngestResize, resize16.ResizeHalf, resample.Resample)


@pytest.fixture
def built(monkeypatch):
    """Canvas and the resize plans record (class, positional arguments, keywords) instead of creating a plan."""
    log = []
    for cls in RESIZES + (canvas.Canvas,):
        def init(self, *args, _cls=cls, **kw):
            log.append((_cls, args, kw))
        monkeypatch.setattr(cls, "__init__", init)
    return log


def _torch_u8():
    import torch
    return torch.uint8


def test_delivery_end_defaults_and_same_aspect_build_no_canvas(built):
    u8 = _torch_u8()
    for kw in (dict(), dict(deliver_fit="stretch", pad_color=(9, 9, 9))):
        for deliver in (None, (36, 64), (40, 40)):
            del built[:]
            end = ends.DeliveryEnd("dev", (72, 128), u8, "rgb24", "bt601", "tv", "center", deliver, "bilinear", **kw)
            assert end.canvas is None and [b[0] for b in built] == ([] if deliver is None else [ingest.IngestResize])
            assert (end.resize is None) == (deliver is None) and end.size == (deliver or (72, 128))
    for fit in ("pad", "crop"):                                                # 16:9 -> 16:9, and an aspect that rounds to the delivery
        for render, deliver in (((72, 128), (36, 64)), ((18, 32), (9, 16)), ((13, 19), (5, 7)) if fit == "pad" else ((18, 32), (27, 48))):
            del built[:]
            end = ends.DeliveryEnd("dev", render, u8, "rgb24", "bt601", "tv", "center", deliver, "lanczos", deliver_fit=fit, pad_color=(1, 2, 3))
            assert end.canvas is None and built == [(resample.Resample, ("dev", render, deliver), {"filter": "lanczos", "dtype": u8})], (fit, built)
            assert [hw for _, hw in end.stages] == [deliver]


def test_delivery_end_pad_and_crop_stages(built):
    import torch
    u8, f16 = torch.uint8, torch.float16
    # pad: 4:3 render in 16:9, inner size other than the render: resize -> inner, Canvas -> delivery
    end = ends.DeliveryEnd("dev", (48, 64), u8, "rgb24", "bt601", "tv", "center", (36, 64), "bilinear", deliver_fit="pad", pad_color=(7, 200, 33))
    assert built == [(ingest.IngestResize, ("dev", (48, 64), (36, 48)), {}),
                         (canvas.Canvas, ("dev", (36, 48), (36, 64)), {"at": (0, 8), "fill": (7, 200, 33), "dtype": u8})]
    assert [hw for _, hw in end.stages] == [(36, 48), (36, 64)] and end.size == (36, 64) and end.frame_bytes == 36 * 64 * 3
    assert end.egress is None and type(end.resize) is ingest.IngestResize and type(end.canvas) is canvas.Canvas
    # pad where the inner size IS the render size: no resize
    del built[:]
    end = ends.DeliveryEnd("dev", (36, 48), f16, "rgb24", "bt601", "tv", "center", (36, 64), "bicubic", deliver_fit="pad")
    assert built == [(canvas.Canvas, ("dev", (36, 48), (36, 64)), {"at": (0, 8), "fill": (0, 0, 0), "dtype": f16})]
    assert end.resize is None and [hw for _, hw in end.stages] == [(36, 64)] and end.shape(3) == (3, 36, 64, 3)
    # crop: 16:9 render for a 4:3 delivery: Canvas cuts the window, resize -> delivery
    del built[:]
    end = ends.DeliveryEnd("dev", (72, 128), f16, "rgb24", "bt601", "tv", "center", (36, 48), "bilinear", deliver_fit="crop", pad_color=(5, 5, 5))
    assert built == [(canvas.Canvas, ("dev", (72, 128), (72, 96)), {"window": (0, 16, 72, 96), "dtype": f16}),
                     (resize16.ResizeHalf, ("dev", (72, 96), (36, 48)), {})]
    assert [hw for _, hw in end.stages] == [(72, 96), (36, 48)]
    # crop where the window has the delivery size: no resize
    del built[:]
    end = ends.DeliveryEnd("dev", (72, 128), u8, "rgb24", "bt601", "tv", "center", (72, 96), "lanczos", deliver_fit="crop")
    assert built == [(canvas.Canvas, ("dev", (72, 128), (72, 96)), {"window": (0, 16, 72, 96), "dtype": u8})] and end.resize is None


def test_source_end_stages(built, monkeypatch):
    import torch
    u8, f16 = torch.uint8, torch.float16

    class Plan:
        frame_bytes = 123
    made = []
    monkeypatch.setattr(formats, "source_plan", lambda *a: made.append(a) or (None if a[2] == "rgb24" else Plan()))
    src = ends.SourceEnd("dev", (24, 32), "rgb24", "bt601", "tv", "replicate", (24, 32), "bilinear")          # the defaults: nothing
    assert src.canvas is None and src.resize is None and built == [] and src.stages == []
    src = ends.SourceEnd("dev", (24, 32), "nv12", "bt601", "tv", "replicate", (48, 64), "bilinear")           # as it was: plan, resize
    assert src.canvas is None and built == [(ingest.IngestResize, ("dev", (48, 64), (24, 32)), {})] and [hw for _, hw in src.stages] == [(48, 64), (24, 32)]
    del built[:]
    src = ends.SourceEnd("dev", (24, 32), "nv12", "bt601", "tv", "replicate", (48, 64), "bicubic", crop=(6, 0, 36, 64))
    assert built == [(canvas.Canvas, ("dev", (48, 64), (36, 64)), {"window": (6, 0, 36, 64), "dtype": u8}),
                     (resample.Resample, ("dev", (36, 64), (24, 32)), {"filter": "bicubic", "dtype": u8})]
    assert [hw for _, hw in src.stages] == [(48, 64), (36, 64), (24, 32)] and src.frame_shape == (123,)
    del built[:]
    src = ends.SourceEnd("dev", (24, 32), "rgb24", "bt601", "tv", "replicate", (30, 40), "bilinear", crop=(3, 4, 24, 32))     # window = render size
    assert built == [(canvas.Canvas, ("dev", (30, 40), (24, 32)), {"window": (3, 4, 24, 32), "dtype": u8})] and src.resize is None
    assert src.plan is None and src.frame_shape == (30, 40, 3) and src.frame_bytes == 30 * 40 * 3
    del built[:]
    src = ends.SourceEnd("dev", (24, 32), "p010le", "bt601", "tv", "replicate", (30, 40), "bilinear", crop=(3, 4, 24, 32), dtype=f16)
    assert built == [(canvas.Canvas, ("dev", (30, 40), (24, 32)), {"window": (3, 4, 24, 32), "dtype": f16})] and src.resize is None
