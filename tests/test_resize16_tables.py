"""The half resampler without a GPU (include/crtfx_resize16.h): the int64 model (tests/resize16_model.py) is tied to the 8-bit model that
equals the installed Pillow byte for byte, and held to a float64 restatement; its quantiser is deep_model's for every half bit pattern; no
accumulator of a real table can wrap; the C-ABI is bound symbol for symbol and refuses bad arguments before it touches a device, as do
process_frames(deliver_size=) and the CLI's --deliver-width / --deliver-height; the builds' registers and LDS are the header's."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pythoncrt_amd import _lib, tables  # noqa: E402
from tests import deep_model, pil_resize_model  # noqa: E402
from tests import resize16_model as model  # noqa: E402

ALL_PAIRS = pil_resize_model.PAIRS + pil_resize_model.EXTRA_PAIRS
AXES = sorted({(s[i], d[i]) for s, d in ALL_PAIRS for i in (0, 1)} | set(model.FULL_AXES))


def _ids(s):
    return f"{s[0]}x{s[1]}"


@pytest.mark.parametrize("src,dst", pil_resize_model.PAIRS, ids=_ids)
def test_the_pass_is_the_one_held_to_pillow(src, dst):
    """resample_pass(top=255) on uint8 images == pil_resize_model.resample_pass, both passes, and the two passes chained == Pillow itself:
    0 bytes differ.  The code that the kernels are compared with is the code that is held to the installed Pillow."""
    ax, ay = tables.pil_resample_axis(src[1], dst[1]), tables.pil_resample_axis(src[0], dst[0])
    for name, img in pil_resize_model.images(*src).items():
        hor = model.resample_pass(img, *ax, top=255)
        ref = pil_resize_model.resample_pass(img, *ax)
        assert hor.dtype == np.int64 and np.array_equal(hor, ref), (src, dst, name)
        ver = model.resample_pass(np.ascontiguousarray(hor.transpose(1, 0, 2)), *ay, top=255)
        assert np.array_equal(ver, pil_resize_model.resample_pass(np.ascontiguousarray(ref.transpose(1, 0, 2)), *ay)), (src, dst, name)
        got = np.ascontiguousarray(ver.transpose(1, 0, 2)).astype(np.uint8)
        exp = pil_resize_model.pillow(img, *dst)
        assert int((got != exp).sum()) == 0, (src, dst, name, int((got != exp).sum()))


@pytest.mark.parametrize("src,dst", ALL_PAIRS, ids=_ids)
def test_model_against_the_float_restatement(src, dst):
    """The model's quarter codes against the exact separable weighted mean with the float weights k / 2^22: at most
    1 + 1.3e-4 * (ksize_x + ksize_y) quarter codes apart — two roundings of a half each, the first carried through convex weights, plus the
    coefficient rounding (a row sums to 2^22 within +-ksize / 2, times 1020) — and the result is a float16 frame of quarter codes."""
    kx, ky = tables.pil_resample_axis(src[1], dst[1])[2].shape[1], tables.pil_resample_axis(src[0], dst[0])[2].shape[1]
    bound = 1.0 + 1.3e-4 * (kx + ky)
    for name, img in model.images(*src).items():
        q = model.quantise(img)
        assert q.min() >= 0 and q.max() <= model.QMAX
        got = model.resize_codes(q, *dst)
        ref = model.resize_float(q, *dst)
        assert got.shape == ref.shape == (dst[0], dst[1], 3)
        err = float(np.abs(got - ref).max())
        assert err <= bound, (src, dst, name, err, bound)
        out = model.resize(img, *dst)
        assert out.dtype == np.float16 and np.array_equal(out.astype(np.float64) * 4.0, got.astype(np.float64))


def test_a_constant_image_stays_constant_and_an_equal_size_is_the_quantiser():
    for q in (0, 1, 511, 1019, 1020):
        img = np.full((13, 17, 3), q / 4.0, dtype=np.float16)
        for dst in ((5, 7), (13, 40), (31, 17), (1, 1)):
            assert (model.resize_codes(model.quantise(img), *dst) == q).all(), (q, dst)
    for src in ((1, 1), (7, 5), (45, 80)):
        img = model.images(*src)["random"]
        out = model.resize(img, *src)
        exp = model.to_half(model.quantise(img))
        assert np.array_equal(out.view(np.uint16), exp.view(np.uint16)), src


def test_quantiser_is_the_egress_stages_for_every_half():
    """All 65 536 bit patterns: resize16_model.quantise == deep_model.quantise; NaN, -0, negatives and -inf give 0, +inf 1020, ties go to even."""
    every = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    q = model.quantise(every)
    assert np.array_equal(q, deep_model.quantise(every)) and q.min() == 0 and q.max() == model.QMAX
    f = every.astype(np.float64)
    assert (q[np.isnan(f)] == 0).all() and (q[f <= 0] == 0).all() and (q[f >= 255.0] == model.QMAX).all()
    assert model.quantise(np.array([0.125, 0.375, 0.625], dtype=np.float16)).tolist() == [0, 2, 2]
    codes = np.arange(model.QMAX + 1)
    assert np.array_equal(model.quantise(model.to_half(codes)), codes)          # every quarter code is exactly a half


@pytest.mark.parametrize("n_in,n_out", AXES, ids=str)
def test_no_accumulator_can_wrap(n_in, n_out):
    """The bound crtfx_resize16_create checks, on the tables of every test pair and of the full-size pairs: a row sums to 2^22 within +-ksize (each
    tap rounds once; in fact within 2^22 - 2 .. 2^22 + 3, the header's figures), so 2^21 + 1020 * sum < 2^32 with room to spare, and every
    coefficient fits the 24-bit multiply."""
    xmin, count, k = tables.pil_resample_axis(n_in, n_out)
    kk = np.where(np.arange(k.shape[1])[None, :] < count[:, None], k, 0).astype(np.int64)
    sums = kk.sum(axis=1)
    assert np.abs(sums - (1 << 22)).max() <= k.shape[1], (int(sums.min()), int(sums.max()))
    assert (1 << 22) - 2 <= int(sums.min()) and int(sums.max()) <= (1 << 22) + 3, (int(sums.min()), int(sums.max()))
    assert (1 << 21) + model.QMAX * int(sums.max()) < 2 ** 32
    assert kk.min() >= 0 and kk.max() < 1 << 24


def test_header_prototypes_are_the_bound_symbols():
    """include/crtfx_resize16.h declares exactly _lib.RESIZE16_SYMBOLS (argument counts included), the shape of the ingest stage's table, and
    the built library exports every one."""
    hdr = open(os.path.join(ROOT, "include", "crtfx_resize16.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(crtfx_resize16_\w+)\s*\(([^)]*)\)\s*;", hdr)}
    assert set(protos) == set(_lib.RESIZE16_SYMBOLS) and len(protos) == 6, set(protos) ^ set(_lib.RESIZE16_SYMBOLS)
    others = (set(_lib.SYMBOLS) | set(_lib.INGEST_SYMBOLS) | set(_lib.EGRESS_SYMBOLS) | set(_lib.UNPACK_SYMBOLS) | set(_lib.DEEP_SYMBOLS) | set(_lib.YUV422_SYMBOLS)
              | set(_lib.DEEP444_SYMBOLS) | set(_lib.SITED_SYMBOLS) | set(_lib.EGRESS_SITED_SYMBOLS))
    assert not set(_lib.RESIZE16_SYMBOLS) & others
    for name, args in protos.items():
        n_args = 0 if args.strip() in ("", "void") else len(args.split(","))
        assert n_args == len(_lib.RESIZE16_SYMBOLS[name][1]), name
        assert _lib.RESIZE16_SYMBOLS[name] == _lib.INGEST_SYMBOLS[name.replace("crtfx_resize16_", "crtfx_ingest_")], name
    assert all(os.path.basename(f) in {os.path.basename(s) for s in _lib.SOURCES} for f in ("crtfx_resize16.hip", "crtfx_resize16.h"))
    assert "crtfx_resize16" in _lib.STAGE_UNITS and _lib.RESIZE16_OPT_FORCE_GENERAL == 1
    lib = _lib.load()
    for name in _lib.RESIZE16_SYMBOLS:
        assert getattr(lib, name).argtypes == _lib.RESIZE16_SYMBOLS[name][1]
    import pythoncrt_amd as pc
    assert pc.ResizeHalf.__name__ in pc.__all__


def _create(lib, src, dst, pix_fmt=_lib.PIX_F16, device=0, mutate=None, null=False, no_out=False):
    ax, ay = tables.pil_resample_axis(src[1], max(1, min(dst[1], 32767))), tables.pil_resample_axis(src[0], max(1, min(dst[0], 32767)))
    if mutate:
        mutate(ax, ay)
    plan = ctypes.c_void_p(1)
    rc = lib.crtfx_resize16_create(device, src[0], src[1], dst[0], dst[1], pix_fmt, None if null else tables.ptr(ax[0]), tables.ptr(ax[1]), tables.ptr(ax[2]),
                                   ax[2].shape[1], tables.ptr(ay[0]), tables.ptr(ay[1]), tables.ptr(ay[2]), ay[2].shape[1],
                                   None if no_out else ctypes.byref(plan))
    return rc, plan, (lib.crtfx_resize16_last_error(None) or b"").decode()


def test_create_refuses_bad_arguments_before_it_touches_a_device():
    """The argument checks of crtfx_resize16_create come first, so they hold on any machine: uint8 frames are UNSUPPORTED (they have the
    ingest stage); sizes 0 and 32768, a null table, a decreasing min, count > ksize, a row whose accumulator could wrap and a null out
    pointer are INVALID; each leaves *out_plan NULL and a message."""
    lib = _lib.load()

    def moves_back(ax, ay):
        ay[0][1] = ay[0][2] + 1

    def count_over_ksize(ax, ay):
        ax[1][3] = ax[2].shape[1] + 1

    def row_wraps(ax, ay):
        ax[2][5, 0] = (1 << 22) + 20000          # 1020 * (2^22 + 20000 + the rest of the row) + 2^21 >= 2^32; each coefficient still < 2^24

    def row_just_fits(ax, ay):
        ax[2][5, :] = 0
        ax[2][5, 0] = ((1 << 32) - (1 << 21) - 1) // 1020

    for kw, code, word in ((dict(pix_fmt=_lib.PIX_U8), _lib.E_UNSUPPORTED, "half"), (dict(dst=(0, 8)), _lib.E_INVALID, "sizes"),
                           (dict(dst=(8, 32768)), _lib.E_INVALID, "sizes"), (dict(dst=(32768, 8)), _lib.E_INVALID, "sizes"),
                           (dict(null=True), _lib.E_INVALID, "null"), (dict(pix_fmt=7), _lib.E_INVALID, "pixel format"),
                           (dict(mutate=moves_back), _lib.E_INVALID, "y tables"), (dict(mutate=count_over_ksize), _lib.E_INVALID, "x tables"),
                           (dict(mutate=row_wraps), _lib.E_INVALID, "wrap")):
        args = dict(src=(12, 20), dst=(30, 31))
        args.update(kw)
        rc, plan, msg = _create(lib, **args)
        assert rc == code and not plan.value and word in msg, (kw, rc, plan.value, msg)
    rc, plan, msg = _create(lib, (12, 20), (30, 31), no_out=True)
    assert rc == _lib.E_INVALID and "out_plan" in msg
    # the largest row that is admitted passes the table checks: what is left to fail without a device is the device itself
    import torch
    if not torch.cuda.is_available():
        rc, plan, msg = _create(lib, (12, 20), (30, 31), mutate=row_just_fits)
        assert rc == _lib.E_HIP and not plan.value and "wrap" not in msg, (rc, msg)
    assert lib.crtfx_resize16_destroy(None) == _lib.OK and lib.crtfx_resize16_set_option(None, 1, 1) == _lib.E_INVALID
    assert lib.crtfx_resize16_run(None, None, 0, None, 0, 1, None) == _lib.E_INVALID
    assert lib.crtfx_resize16_last_plan(None, ctypes.create_string_buffer(8), 8) == _lib.E_INVALID


def test_create_without_a_gpu_fails_cleanly():
    import torch
    lib = _lib.load()
    if torch.cuda.is_available():
        rc, plan, msg = _create(lib, (12, 20), (30, 31), device=4096)              # no such device on any box
        assert rc == _lib.E_HIP and not plan.value and "4096" in msg
        return
    rc, plan, msg = _create(lib, (12, 20), (30, 31))
    assert rc == _lib.E_HIP and not plan.value and msg, (rc, msg)


def test_process_frames_refuses_a_bad_deliver_size_before_a_device_is_touched(monkeypatch):
    """A size < 1 or > 32767 and a value that is not a pair are ValueError, raised before a frame is read and before the device is asked
    for (torch.cuda.is_available is made to fail the test if it is reached)."""
    import torch
    import pythoncrt_amd as pc
    from pythoncrt_amd import render

    def never():
        raise AssertionError("a frame was read")
        yield

    def no_device():
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    for bad in ((0, 40), (23, 0), (-1, 5), (32768, 40), (23, 32768), 40, (23,), (23, 40, 3), "ab", (23.5, 40), (None, 40)):
        for fmts in ({}, dict(in_pix_fmt="p010le", out_pix_fmt="p010le")):
            with pytest.raises(ValueError, match="deliver_size"):
                pc.process_frames(never(), lambda a: None, 80, 46, 30.0, 1, deliver_size=bad, **fmts)
    assert render.parse_deliver_size(None, 46, 80) is None and render.parse_deliver_size((46, 80), 46, 80) is None
    assert render.parse_deliver_size((23, 40), 46, 80) == (23, 40) and render.parse_deliver_size([32767, 1], 46, 80) == (32767, 1)
    assert render.parse_deliver_size(np.array([23, 40]), 46, 80) == (23, 40)


def test_cli_delivery_flags_go_together_and_the_sharded_cli_refuses_them(tmp_path, monkeypatch):
    from pythoncrt_amd import cli
    src = tmp_path / "in.rgb"
    src.write_bytes(bytes(46 * 80 * 3))
    base = ["--input", str(src), "--output", str(tmp_path / "out.rgb"), "--width", "80", "--height", "46"]
    for extra in (["--deliver-width", "40"], ["--deliver-height", "23"], ["--deliver-width", "40", "--deliver-height", "0"]):
        with pytest.raises(SystemExit) as e:
            cli.main(base + extra)
        assert e.value.code not in (0, None) and "--deliver-width and --deliver-height" in str(e.value), extra
    with pytest.raises(SystemExit) as e:
        cli.main(base + ["--deliver-width", "40000", "--deliver-height", "23"])
    assert "32767" in str(e.value)
    assert not (tmp_path / "out.rgb").exists()
    a = cli.add_input_flags(cli.add_output_flags(cli.build_parser())).parse_args(base)
    assert (a.deliver_width, a.deliver_height) == (0, 0) and cli.deliver_size_from_args(a) is None                   # neither: as rendered
    a = cli.add_input_flags(cli.add_output_flags(cli.build_parser())).parse_args(base + ["--deliver-width", "80", "--deliver-height", "46"])
    assert cli.deliver_size_from_args(a) is None                                                                   # the render size: as rendered
    a = cli.add_input_flags(cli.add_output_flags(cli.build_parser())).parse_args(base + ["--deliver-width", "40", "--deliver-height", "23"])
    assert cli.deliver_size_from_args(a) == (23, 40)
    monkeypatch.setenv("CRTFX_FORCE_DIST", "1")
    with pytest.raises(SystemExit) as e:
        cli.main(base + ["--deliver-width", "40", "--deliver-height", "23"])
    assert e.value.code not in (0, None) and "sharded CLI" in str(e.value) and "--deliver-width" in str(e.value)
    assert not (tmp_path / "out.rgb").exists()


# what include/crtfx_resize16.h states for the three builds: VGPRs as built
HEADER_VGPRS = {"k_resize16_fused": 43, "k_resize16_h": 32, "k_resize16_v": 6}


def test_resize16_kernels_hold_the_register_budget_and_the_header():
    """Registers and scratch of the three kernels, read from the built library's code objects (tools/kernel_resources.py): at most 128 VGPRs
    (in fact at most 64: eight waves per SIMD), no AGPRs, no spills, no scratch memory, no static LDS (the fused kernel's block is dynamic:
    its size is the plan's `lds`) — and the figures the header quotes are the figures of this build."""
    import kernel_resources
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    res = kernel_resources.resources(_lib.LIB_PATH)
    found = {n.split("::")[1]: v for n, v in res.items() if n.startswith("crtfx_resize16_impl::")}
    assert set(found) == set(HEADER_VGPRS), sorted(found)
    hdr = open(os.path.join(ROOT, "include", "crtfx_resize16.h")).read()
    for name, v in found.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["group_segment_fixed_size"] == 0 and v["agpr_count"] == 0 and v["vgpr_count"] <= 128, (name, v)
        assert v["vgpr_count"] == HEADER_VGPRS[name], (name, v["vgpr_count"])
        assert re.search(rf"{name} {HEADER_VGPRS[name]}\b", hdr), name
    assert "40 960" in hdr and "(32,128) (32,64) (16,128) (16,64) (8,64) (8,32) (4,32)" in hdr
