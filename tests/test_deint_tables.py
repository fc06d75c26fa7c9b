"""The deinterlace stage without a GPU (include/crtfx_deint.h): the model's properties (kept rows are bits, constants and ramps survive,
EDGE against LINEAR, stripes, the spread of directions on noise, the half quantiser and its bounds, BOTH against FIRST), the C-ABI bound
symbol for symbol and refusing bad arguments before it touches a device, every refusal of process_frames(deinterlace=) and of the CLI's
flags, the stages SourceEnd builds with and without the keyword, and the builds' registers against the header."""
import ctypes
import itertools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pythoncrt_amd import _lib, _stage, canvas, deint, depth, ends, formats, ingest, resample, resize16  # noqa: E402
from tests import deint_model as model  # noqa: E402
from tests import resize16_model  # noqa: E402

HEADER = os.path.join(ROOT, "include", "crtfx_deint.h")
DTYPES = (np.uint8, np.float16)
COMBOS = list(itertools.product(model.METHODS, model.ORDERS, model.FIELDS))


def _all_halves():
    return np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)


def _kept(order, fields, j):
    """The field whose rows output frame j of a source frame keeps."""
    first = model.ORDERS.index(order)
    return first if fields == "first" or j == 0 else 1 - first


# ---- the arithmetic -------------------------------------------------------------------------------------------------------------------------

def test_names_are_one_list_in_the_model_and_the_module():
    assert deint.METHODS == model.METHODS == ("linear", "edge")
    assert deint.ORDERS == model.ORDERS == ("tff", "bff") and deint.FIELDS == model.FIELDS == ("first", "both")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method,order,fields", COMBOS)
def test_kept_rows_are_the_sources_bits(dtype, method, order, fields):
    src = model.noise(9, 12, n=2, dtype=dtype, seed=3)
    if dtype == np.float16:                                                     # patterns the arithmetic would change: NaNs with payloads, -0, negatives, > 255
        src = src.copy()
        src.view(np.uint16)[:, :, :4, :] = np.array([0x7e01, 0xfc01, 0x8000, 0xc500, 0x7bff, 0x0001, 0x7c00, 0xfe55, 0x3555, 0x5bf9, 0x5c01, 0x7fff],
                                                    dtype=np.uint16).reshape(4, 3)
    out = model.deinterlace(src, method, order, fields)
    per = len(model.FIELDS[:model.FIELDS.index(fields) + 1])
    assert out.shape == (2 * per, 9, 12, 3) and out.dtype == dtype
    for j in range(out.shape[0]):
        f = _kept(order, fields, j % per)
        assert np.array_equal(model.bits(out[j, f::2]), model.bits(src[j // per, f::2]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method,order,fields", COMBOS)
def test_a_constant_frame_stays_constant(dtype, method, order, fields):
    for h, w in ((2, 1), (3, 7), (8, 16)):
        src = np.empty((1, h, w, 3), dtype=dtype)
        src[...] = np.array([17, 200.25 if dtype == np.float16 else 200, 255], dtype=dtype)
        out = model.deinterlace(src, method, order, fields)
        assert (out == src[0, 0, 0]).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_vertical_ramp_comes_back_under_linear(dtype):
    h, w = 11, 9
    src = np.broadcast_to((np.arange(h) * 7 + 3)[:, None, None], (h, w, 3)).astype(dtype)[None]
    for order, fields in itertools.product(model.ORDERS, model.FIELDS):
        out = model.deinterlace(src, "linear", order, fields)
        assert np.array_equal(out[:, 1:-1], np.broadcast_to(src[:, 1:-1], out[:, 1:-1].shape))      # (a + b + 1) >> 1 of y - 1 and y + 1 is y
        for j in range(out.shape[0]):                                           # the first and the last row: kept, or a copy of the one neighbour
            f = _kept(order, fields, j)
            assert np.array_equal(out[j, 0], src[0, 0 if f == 0 else 1]) and np.array_equal(out[j, -1], src[0, h - 1 if (h - 1) % 2 == f else h - 2])


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_is_linear_where_d_is_zero_and_on_narrow_frames(dtype):
    src = model.noise(23, 40, n=2, dtype=dtype)
    for order, fields in itertools.product(model.ORDERS, model.FIELDS):
        e, d = model.deinterlace_d(src, "edge", order, fields)
        lin = model.deinterlace(src, "linear", order, fields)
        same = np.broadcast_to((d == 0)[..., None], e.shape)
        assert np.array_equal(model.bits(e)[same], model.bits(lin)[same]) and (d != 0).any()
        assert (d[:, :, :3] == 0).all() and (d[:, :, -3:] == 0).all() and (d[:, 0] == 0).all() and (d[:, -1] == 0).all() and np.abs(d).max() == 2
    for w in range(1, 7):                                                       # narrower than 7: no column has x >= 3 and x <= w - 4
        src = model.noise(6, w, dtype=dtype, seed=w)
        e, d = model.deinterlace_d(src, "edge", "tff", "both")
        assert not d.any() and np.array_equal(model.bits(e), model.bits(model.deinterlace(src, "linear", "tff", "both")))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("slope", [-2, -1, 1, 2])
def test_stripes_choose_their_slope(dtype, slope):
    src = model.stripes(6, 24, slope, dtype)
    out, d = model.deinterlace_d(src, "edge", "tff", "both")
    for j, f in enumerate((0, 1)):
        rows = [y for y in range(1, 5) if y % 2 != f]
        assert (d[j, rows, 3:-3] == slope).all(), d[j]
        assert np.array_equal(out[j, rows, 3:-3], src[0, rows, 3:-3])           # along the stripe the two kept pixels ARE the missing one


def test_noise_takes_every_direction():
    """The seeded 23 x 40 noise frame test_deint_gpu.py runs: each of the five directions on at least 5 % of the interior missing pixels, so
    a kernel that always took d = 0 could not pass there."""
    for dtype in DTYPES:
        src = model.noise(23, 40, dtype=dtype)
        for order in model.ORDERS:
            _, d = model.deinterlace_d(src, "edge", order, "first")
            f = model.ORDERS.index(order)
            rows = [y for y in range(1, 22) if y % 2 != f]
            inner = d[0, rows, 3:-3]
            share = {j: float((inner == j).mean()) for j in (-2, -1, 0, 1, 2)}
            assert min(share.values()) >= 0.05 and abs(sum(share.values()) - 1) < 1e-12, share


def test_the_half_quantiser_and_its_bounds():
    halves = _all_halves()
    q = model.quantise(halves)
    assert np.array_equal(q, resize16_model.quantise(halves)) and q.min() == 0 and q.max() == model.QMAX == 1020
    back = model.from_codes(np.arange(1021), np.float16)                        # every quarter code is a half: nothing is rounded
    assert np.array_equal(back.astype(np.float64) * 4, np.arange(1021)) and np.array_equal(model.quantise(back), np.arange(1021))
    # the accumulator: nine pairs at the two ends of the scale
    a = np.zeros((7, 3), dtype=np.int64)
    b = np.full((7, 3), 1020, dtype=np.int64)
    assert model.score(a, b, 0)[3] == 9 * 1020 and 9 * 1020 < 2 ** 15
    # every result is a quarter code, whatever goes in: all 65 536 patterns in the rows that feed the interpolation
    src = np.zeros((1, 3, 65536 // 3 + 1, 3), dtype=np.float16)
    src.view(np.uint16)[0, 0].reshape(-1)[:65536] = np.arange(65536, dtype=np.uint16)
    src.view(np.uint16)[0, 2].reshape(-1)[:65536] = np.arange(65536, dtype=np.uint16)[::-1]
    for method in model.METHODS:
        out = model.deinterlace(src, method, "tff", "first")[0, 1].astype(np.float64) * 4
        assert np.array_equal(out, np.rint(out)) and out.min() >= 0 and out.max() <= 1020


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", model.METHODS)
def test_both_is_first_of_the_two_orders(dtype, method):
    src = model.noise(10, 17, n=3, dtype=dtype, seed=9)
    t, b = model.deinterlace(src, method, "tff", "first"), model.deinterlace(src, method, "bff", "first")
    both_t, both_b = model.deinterlace(src, method, "tff", "both"), model.deinterlace(src, method, "bff", "both")
    assert np.array_equal(model.bits(both_t[0::2]), model.bits(t)) and np.array_equal(model.bits(both_t[1::2]), model.bits(b))
    assert np.array_equal(model.bits(both_b[0::2]), model.bits(b)) and np.array_equal(model.bits(both_b[1::2]), model.bits(t))
    assert model.deinterlace(src[:0], method, "tff", "both").shape == (0, 10, 17, 3)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------------------

_vp = ctypes.c_void_p
SIGNATURES = {
    "crtfx_deint_create": (ctypes.c_int, [ctypes.c_int] * 7 + [ctypes.POINTER(_vp)]),
    "crtfx_deint_destroy": (ctypes.c_int, [_vp]),
    "crtfx_deint_last_error": (ctypes.c_char_p, [_vp]),
    "crtfx_deint_frames_out": (ctypes.c_int, [_vp]),
    "crtfx_deint_run": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_int, _vp]),
    "crtfx_deint_set_option": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "crtfx_deint_last_plan": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_size_t]),
}


def test_symbols_are_bound_and_the_header_declares_them():
    assert _lib.DEINT_SYMBOLS == SIGNATURES and _lib.DEINT_OPT_FORCE_GENERAL == 1
    assert (_lib.DEINT_LINEAR, _lib.DEINT_EDGE, _lib.DEINT_TFF, _lib.DEINT_BFF, _lib.DEINT_FIRST, _lib.DEINT_BOTH) == (0, 1, 0, 1, 0, 1)
    lib = _lib.load()
    for name, (res, args) in SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res, name
    hdr = open(HEADER).read()
    for text in ("CRTFX_DEINT_OPT_FORCE_GENERAL = 1", "CRTFX_DEINT_LINEAR = 0", "CRTFX_DEINT_EDGE = 1", "CRTFX_DEINT_TFF = 0", "CRTFX_DEINT_BFF = 1",
                 "CRTFX_DEINT_FIRST = 0", "CRTFX_DEINT_BOTH = 1", "NOT claimed is equality with any other deinterlacer", "No clamp is needed"):
        assert text in hdr, text
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(crtfx_deint_\w+)\s*\(([^)]*)\)\s*;", hdr)}
    assert set(protos) == set(SIGNATURES) and len(protos) == 7, set(protos) ^ set(SIGNATURES)
    for name, args in protos.items():
        assert len(args.split(",")) == len(SIGNATURES[name][1]), name
    order = [a.split()[-1].lstrip("*") for a in protos["crtfx_deint_create"].split(",")]
    assert order == ["device", "h", "w", "pix_fmt", "method", "order", "fields", "out_plan"]
    others = set()
    for table in ("SYMBOLS", "INGEST_SYMBOLS", "EGRESS_SYMBOLS", "UNPACK_SYMBOLS", "DEEP_SYMBOLS", "YUV422_SYMBOLS", "DEEP444_SYMBOLS", "SITED_SYMBOLS",
                  "EGRESS_SITED_SYMBOLS", "RESIZE16_SYMBOLS", "RESAMPLE_SYMBOLS", "CANVAS_SYMBOLS", "DEPTH_SYMBOLS"):
        others |= set(getattr(_lib, table))
    assert not set(SIGNATURES) & others
    assert all(os.path.basename(f) in {os.path.basename(s) for s in _lib.SOURCES} for f in ("crtfx_deint.hip", "crtfx_deint.h"))
    assert all(os.path.exists(s) for s in _lib.SOURCES) and "crtfx_deint" in _lib.STAGE_UNITS
    import pythoncrt_amd as pc
    assert pc.Deinterlace is deint.Deinterlace and "Deinterlace" in pc.__all__ and issubclass(pc.Deinterlace, _stage.Handle)
    import bench                                                               # a namespace of its own, outside the chain's evidence hash
    assert "crtfx_deint" not in open(bench.__file__).read()
    assert "namespace crtfx_deint_impl" in open(os.path.join(_lib.CSRC, "crtfx_deint.hip")).read()


GOOD = dict(device=0, h=9, w=24, pix_fmt=_lib.PIX_U8, method=_lib.DEINT_EDGE, order=_lib.DEINT_BFF, fields=_lib.DEINT_BOTH)


def _create(lib, no_out=False, **kw):
    a = dict(GOOD)
    a.update(kw)
    plan = ctypes.c_void_p(1)
    rc = lib.crtfx_deint_create(*(a[k] for k in GOOD), None if no_out else ctypes.byref(plan))
    return rc, plan, (lib.crtfx_deint_last_error(None) or b"").decode()


def test_create_refuses_bad_arguments_before_it_touches_a_device():
    """Every refusal of crtfx_deint_create comes before the device is asked for, so it holds on any machine; *out_plan is NULL and the
    message names the offending field.  The call that passes every check is left with the device: `no HIP device 4096`."""
    lib = _lib.load()
    cases = [(dict(h=v), "h =") for v in (1, 0, -3, 32768)] + [(dict(w=v), "w =") for v in (0, -3, 32768)]
    cases += [({k: v}, k) for k in ("pix_fmt", "method", "order", "fields") for v in (2, -1, 7)]
    for kw, word in cases:
        rc, plan, msg = _create(lib, **kw)
        assert rc == _lib.E_INVALID and not plan.value and word in msg, (kw, rc, plan.value, msg)
    rc, plan, msg = _create(lib, no_out=True)
    assert rc == _lib.E_INVALID and "out_plan" in msg
    for kw in (dict(), dict(h=2, w=1), dict(h=32767, w=32767, pix_fmt=_lib.PIX_F16), dict(method=0, order=0, fields=0)):
        rc, plan, msg = _create(lib, device=4096, **kw)
        assert rc == _lib.E_HIP and not plan.value and "no HIP device 4096" in msg, (kw, rc, msg)
    assert lib.crtfx_deint_destroy(None) == _lib.OK and lib.crtfx_deint_set_option(None, 1, 1) == _lib.E_INVALID
    assert lib.crtfx_deint_frames_out(None) == 0
    assert lib.crtfx_deint_run(None, None, 0, None, 0, 1, None) == _lib.E_INVALID
    assert lib.crtfx_deint_last_plan(None, ctypes.create_string_buffer(8), 8) == _lib.E_INVALID


def test_python_plan_refuses_before_a_device():
    for kw in (dict(method="yadif"), dict(order="top"), dict(fields="second"), dict(method=None), dict(fields=2)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            deint.Deinterlace("cpu", (4, 4), **kw)
    with pytest.raises(ValueError, match="ROCm device"):
        deint.Deinterlace("cpu", (4, 4))


# what include/crtfx_deint.h states for the sixteen builds: VGPRs as built
HEADER_VGPRS = {
    "k_deint<linear,u8,first,vec>": 18, "k_deint<linear,u8,both,vec>": 22, "k_deint<linear,f16,first,vec>": 31, "k_deint<linear,f16,both,vec>": 32,
    "k_deint<edge,u8,first,vec>": 89, "k_deint<edge,u8,both,vec>": 91, "k_deint<edge,f16,first,vec>": 127, "k_deint<edge,f16,both,vec>": 129,
    "k_deint<linear,u8,first,general>": 10, "k_deint<linear,u8,both,general>": 9, "k_deint<linear,f16,first,general>": 11,
    "k_deint<linear,f16,both,general>": 9, "k_deint<edge,u8,first,general>": 59, "k_deint<edge,u8,both,general>": 59,
    "k_deint<edge,f16,first,general>": 60, "k_deint<edge,f16,both,general>": 60}


def test_deint_kernels_have_no_scratch_and_the_headers_registers():
    """Registers, LDS and scratch of the sixteen builds, read from the built library's code objects (tools/kernel_resources.py): no LDS, no
    scratch memory, no spills, no AGPRs — and the figures the header quotes are the figures of this build."""
    import kernel_resources
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    res = kernel_resources.resources(_lib.LIB_PATH)
    found = {n.replace("crtfx_deint_impl::", "").replace(", ", ","): v for n, v in res.items() if n.startswith("crtfx_deint_impl::")}
    assert set(found) == set(HEADER_VGPRS), sorted(found)
    hdr = open(HEADER).read()
    for name, v in found.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["group_segment_fixed_size"] == 0 and v["agpr_count"] == 0, (name, v)
        assert v["vgpr_count"] == HEADER_VGPRS[name], (name, v["vgpr_count"])
        assert re.search(rf"{re.escape(name)} {HEADER_VGPRS[name]}\b", hdr), name
    assert "no AGPRs, no LDS, no scratch, no spills" in hdr


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
    import pythoncrt_amd as pc
    run = _refusing_process_frames(monkeypatch)
    for bad in ("yadif", "", None, "LINEAR", True, 1):
        with pytest.raises(ValueError, match="deinterlace must be"):
            run(deinterlace=bad)
    for bad in ("top", "", None, "TFF", 0):
        for method in ("off", "linear"):
            with pytest.raises(ValueError, match="field_order must be"):
                run(deinterlace=method, field_order=bad)
    for bad in ("second", "", None, "BOTH", 2):
        for method in ("off", "edge"):
            with pytest.raises(ValueError, match="deinterlace_fields must be"):
                run(deinterlace=method, deinterlace_fields=bad)
    for kw in (dict(field_order="bff"), dict(deinterlace_fields="both"), dict(field_order="bff", deinterlace_fields="both", deinterlace="off")):
        with pytest.raises(ValueError, match="nothing to\\s+deinterlace"):
            run(**kw)
    for method in model.METHODS:
        with pytest.raises(ValueError, match="resize_on='host' cannot be combined with deinterlace"):
            run(deinterlace=method, resize_on="host")
        for kw in (dict(in_size=(1, 80)), dict(in_size=(1, 80), in_pix_fmt="nv12"), dict(in_size=(0, 80), in_pix_fmt="uyvy422")):
            with pytest.raises(ValueError, match="no two fields"):
                run(deinterlace=method, **kw)
    with pytest.raises(ValueError, match="no two fields"):                      # a packed format at a render size of one row
        pc.process_frames(iter(()), lambda a: None, 80, 1, 30.0, 1, deinterlace="linear", in_pix_fmt="uyvy422")
    # what is admitted: the next thing asked for is the device
    for kw in (dict(deinterlace="linear"), dict(deinterlace="edge", field_order="bff", deinterlace_fields="both"),
               dict(deinterlace="edge", in_pix_fmt="nv12", in_size=(50, 90)), dict(deinterlace="linear", in_pix_fmt="p010le", out_pix_fmt="yuv420p10le"),
               dict(deinterlace="linear", in_crop=(3, 0, 20, 40)), dict(deinterlace="edge", chain_pix="half", deinterlace_fields="both"),
               dict(deinterlace="off"), dict(deinterlace="off", field_order="tff", deinterlace_fields="first")):
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
    refused(["--field-order", "bff"], "--field-order bff", "nothing to deinterlace")
    refused(["--deinterlace-fields", "both"], "--deinterlace-fields both", "nothing to deinterlace")
    refused(["--deinterlace", "off", "--field-order", "bff", "--deinterlace-fields", "both"], "nothing to deinterlace")
    one_row = ["--input", str(src), "--output", str(out), "--width", "80", "--height", "1"]
    for method in model.METHODS:
        refused(["--deinterlace", method], "--deinterlace " + method, "no two fields", args=one_row)
    for extra in (["--deinterlace", "yadif"], ["--field-order", "top"], ["--deinterlace-fields", "second"], ["--deinterlace"]):
        with pytest.raises(SystemExit):                                         # argparse's own refusal of an unknown choice
            cli.main(base + extra)
    assert not any(act.dest in ("deinterlace", "field_order", "deinterlace_fields") for act in cli.build_parser()._actions)
    assert not any(act.dest in ("deinterlace", "field_order", "deinterlace_fields") for act in cli.add_output_flags(cli.build_parser())._actions)
    parse = cli.add_input_flags(cli.add_output_flags(cli.build_parser())).parse_args
    a = parse(base)
    spec, ranks = cli.check_flags(a)
    assert (a.deinterlace, a.field_order, a.deinterlace_fields) == ("off", "tff", "first") and spec.deinterlace is None
    assert spec.deliver is None and spec.half is False and ranks is None
    a = parse(base + ["--deinterlace", "edge", "--field-order", "bff", "--deinterlace-fields", "both"])
    spec, ranks = cli.check_flags(a)
    assert spec.deinterlace == ("edge", "bff", "both") and spec.deliver is None and spec.half is False and ranks is None
    assert "--deinterlace edge" in cli.__doc__ and "uyvy422" in cli.__doc__ and "--fps 60" in cli.__doc__
    monkeypatch.setenv("CRTFX_FORCE_DIST", "1")
    refused(["--deinterlace", "linear"], "sharded CLI", "--deinterlace")
    refused(["--deinterlace", "edge", "--deinterlace-fields", "both"], "sharded CLI", "--deinterlace")
    refused(["--field-order", "bff"], "nothing to deinterlace")


# ---- which stages SourceEnd builds ------------------------------------------------------------------------------------------------------------

RESIZES = (ingest.IngestResize, resize16.ResizeHalf, resample.Resample)


@pytest.fixture
def built(monkeypatch):
    """Canvas, the resize plans, Widen and Deinterlace record (class, positional arguments, keywords) instead of creating a plan."""
    log = []
    for cls in RESIZES + (canvas.Canvas, depth.Widen, deint.Deinterlace):
        def init(self, *args, _cls=cls, **kw):
            log.append((_cls, args, kw))
        monkeypatch.setattr(cls, "__init__", init)
    return log


def test_source_end_stages(built, monkeypatch):
    import torch
    u8, f16 = torch.uint8, torch.float16

    class Plan:
        frame_bytes = 123
    monkeypatch.setattr(formats, "source_plan", lambda *a: None if a[2] == "rgb24" else Plan())
    R, S = (24, 32), (48, 64)
    # without the keyword, and with None: what was built before
    for kw in (dict(), dict(deinterlace=None)):
        del built[:]
        src = ends.SourceEnd("dev", R, "rgb24", "bt601", "tv", "replicate", R, "bilinear", **kw)
        assert built == [] and src.stages == [] and src.deint is None and src.ratio == 1
        src = ends.SourceEnd("dev", R, "nv12", "bt601", "tv", "replicate", S, "bicubic", (6, 0, 36, 64), **kw)
        assert [b[0] for b in built] == [canvas.Canvas, resample.Resample] and src.deint is None and src.ratio == 1
        assert [hw for _, hw in src.stages] == [S, (36, 64), R]
    # rgb24 at render size: the Deinterlace is the only stage and writes the chain's input
    for fields, ratio in (("first", 1), ("both", 2)):
        del built[:]
        src = ends.SourceEnd("dev", R, "rgb24", "bt601", "tv", "replicate", R, "bilinear", deinterlace=("edge", "bff", fields))
        assert built == [(deint.Deinterlace, ("dev", R), {"method": "edge", "order": "bff", "fields": fields, "dtype": u8})]
        assert [hw for _, hw in src.stages] == [R] and src.stages[0][0] is src.deint and src.ratio == ratio and src.frame_shape == R + (3,)
    # an off-size packed source with a crop: plan, Deinterlace at the SOURCE size, Canvas, resize
    del built[:]
    src = ends.SourceEnd("dev", R, "nv12", "bt601", "tv", "replicate", S, "bilinear", (6, 0, 36, 64), deinterlace=("linear", "tff", "both"))
    assert built == [(deint.Deinterlace, ("dev", S), {"method": "linear", "order": "tff", "fields": "both", "dtype": u8}),
                     (canvas.Canvas, ("dev", S, (36, 64)), {"window": (6, 0, 36, 64), "dtype": u8}), (ingest.IngestResize, ("dev", (36, 64), R), {})]
    assert [type(st) for st, _ in src.stages] == [Plan, deint.Deinterlace, canvas.Canvas, ingest.IngestResize]
    assert [hw for _, hw in src.stages] == [S, S, (36, 64), R] and src.ratio == 2 and src.frame_shape == (123,)
    # a 10-bit source: on half frames; under a widening chain: on the uint8 frames in front of the Widen
    del built[:]
    src = ends.SourceEnd("dev", R, "p010le", "bt601", "tv", "replicate", R, "bilinear", None, f16, deinterlace=("edge", "tff", "first"))
    assert built == [(deint.Deinterlace, ("dev", R), {"method": "edge", "order": "tff", "fields": "first", "dtype": f16})] and src.ratio == 1
    del built[:]
    src = ends.SourceEnd("dev", R, "rgb24", "bt601", "tv", "replicate", S, "bilinear", None, f16, widen=True, deinterlace=("linear", "bff", "both"))
    assert [b[0] for b in built] == [deint.Deinterlace, ingest.IngestResize, depth.Widen] and built[0][2]["dtype"] == u8 and built[0][1] == ("dev", S)
    assert [hw for _, hw in src.stages] == [S, R, R] and src.ratio == 2


def test_source_end_buffers_hold_ratio_frames_behind_the_deinterlace(built, monkeypatch):
    """slots(B): the staged slots hold B SOURCE frames, a stage in front of the Deinterlace writes B frames, the Deinterlace and every stage
    behind it B * ratio; convert(d, n, dst) hands each stage the frames of the one in front and the last one `dst`."""
    import torch

    class Plan:
        frame_bytes = 123
    monkeypatch.setattr(formats, "source_plan", lambda *a: Plan())
    shapes = []
    real_empty = torch.empty

    def empty(shape, dtype=None, device=None):
        shapes.append((tuple(shape), device))
        return real_empty(shape, dtype=dtype)                                   # on the host: the shapes are what is checked
    monkeypatch.setattr(torch, "empty", empty)
    src = ends.SourceEnd("dev", (24, 32), "nv12", "bt601", "tv", "replicate", (48, 64), "bilinear", deinterlace=("linear", "tff", "both"))
    src.slots(4, 2, pinned=False)
    assert [s for s, dev in shapes if dev == "dev"] == [(4, 48, 64, 3)] * 2 + [(8, 48, 64, 3)] * 2 + [(4, 123)] * 2
    calls = []
    for st, _ in src.stages:
        st.run = lambda x, out, _st=st: calls.append((type(_st), tuple(x.shape), tuple(out.shape))) or out
    dst = real_empty((6, 24, 32, 3), dtype=torch.uint8)
    src.convert(1, 3, dst)
    assert calls == [(Plan, (3, 123), (3, 48, 64, 3)), (deint.Deinterlace, (3, 48, 64, 3), (6, 48, 64, 3)),
                     (ingest.IngestResize, (6, 48, 64, 3), (6, 24, 32, 3))]
