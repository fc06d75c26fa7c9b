"""The depth stage without a GPU (include/crtfx_depth.h): the Bayer matrix in its three places, the exactness of the dither's float32 sum over
every half and every threshold, the model's values on the special halves and its round trip, tile means and the half-code frame, the C-ABI
bound symbol for symbol and refusing bad arguments before it touches a device, every refusal of process_frames(chain_pix=, dither=) and of
the CLI's flags, the stages the two chain ends build for every pairing of depths, and the builds' registers against the header."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pythoncrt_amd import _lib, _stage, canvas, depth, ends, formats, ingest, resample, resize16  # noqa: E402
from tests import depth_model as model  # noqa: E402

HEADER = os.path.join(ROOT, "include", "crtfx_depth.h")


def _all_halves():
    return np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)


# ---- the matrix ---------------------------------------------------------------------------------------------------------------------------

def test_bayer8_is_one_matrix_in_the_model_the_module_and_the_header():
    hdr = open(HEADER).read()
    m = re.search(r"#define\s+CRTFX_DEPTH_BAYER8\s*\{(.*?)\}", hdr, re.S)
    assert m, "no literal CRTFX_DEPTH_BAYER8 table in the header"
    lit = [int(v) for v in re.findall(r"\d+", m.group(1))]
    assert len(lit) == 64
    lit = np.array(lit).reshape(8, 8)
    assert np.array_equal(lit, model.BAYER8) and np.array_equal(np.array(depth.BAYER8), model.BAYER8)
    assert sorted(model.BAYER8.ravel().tolist()) == list(range(64))
    assert model.BAYER8[:2, :2].tolist() == [[0, 32], [48, 16]]                # 16 * [0 2; 3 1]: the recursion's outermost level
    assert np.array_equal(model.bayer(2), [[0, 2], [3, 1]]) and np.array_equal(model.bayer(4), [[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]])
    assert depth.DITHERS == ("none", "ordered") == model.DITHERS
    t = model.thresholds()
    assert t.dtype == np.float32 and t.min() == 1 / 128 and t.max() == 127 / 128 and np.array_equal(t * 128, 2 * model.BAYER8 + 1)


# ---- the arithmetic -------------------------------------------------------------------------------------------------------------------------

def test_the_dither_sum_is_exact_for_every_half_and_every_threshold():
    """All 65 536 half bit patterns x all 64 thresholds: the float32 sum v + t equals the float64 sum, so the floor is the only rounding;
    the results lie in 0..255."""
    v = model.clamp(_all_halves())                                            # float32 [65536]
    assert v.min() == 0 and v.max() == 255 and not np.isnan(v).any()
    t = model.thresholds().ravel()
    s32 = v[:, None] + t[None, :]
    assert s32.dtype == np.float32
    s64 = v.astype(np.float64)[:, None] + t.astype(np.float64)[None, :]
    assert np.array_equal(s32.astype(np.float64), s64)
    u = np.floor(s64)
    assert u.min() == 0 and u.max() == 255
    # ... and the model's own narrowing of those patterns, laid out so that every pattern meets every threshold, is that floor
    frame = np.broadcast_to(_all_halves().reshape(8192, 1, 8, 1), (8192, 8, 8, 8)).reshape(65536, 64, 1)     # pattern p fills the tile at rows 8 (p / 8).., columns 8 (p % 8)..
    got = model.narrow(frame, "ordered")
    exp = u.reshape(8192, 8, 8, 8).transpose(0, 2, 1, 3).reshape(65536, 64, 1).astype(np.uint8)      # [p / 8, p % 8, y, x] -> [p / 8, y, p % 8, x]
    assert got.dtype == np.uint8 and np.array_equal(got, exp)


def test_special_halves():
    f = np.array([np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, -1.0, -6e-8, 6e-8, 255.0, 255.5, 256.0, 65504.0, 254.5, 0.5, 1.5, 2.5], dtype=np.float16)
    frame = np.broadcast_to(f[:, None, None, None], (f.size, 8, 8, 3))
    none = model.narrow(frame, "none")
    assert none[:, 0, 0, 0].tolist() == [0, 0, 255, 0, 0, 0, 0, 0, 0, 255, 255, 255, 255, 254, 0, 2, 2]
    assert (none == none[:, :1, :1, :1]).all()
    o = model.narrow(frame, "ordered")
    for i in (0, 1, 3, 4, 5, 6, 7):                                            # NaN, -inf, -0, 0, negatives: 0 under every threshold (t < 1)
        assert (o[i] == 0).all(), i
    for i in (2, 9, 10, 11, 12):                                               # +inf and everything from 255 up: 255, never 256
        assert (o[i] == 255).all(), i
    assert (o[8] == 0).all()                                                   # the smallest subnormal: 2^-24 + 127 / 128 < 1
    assert set(np.unique(o[13]).tolist()) == {254, 255} and set(np.unique(o[14]).tolist()) == {0, 1}


@pytest.mark.parametrize("dither", model.DITHERS)
def test_narrow_of_widen_is_the_identity(dither):
    u = np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None, None], (256, 8, 8, 3))
    w = model.widen(u)
    assert w.dtype == np.float16 and np.array_equal(w.astype(np.float64), u.astype(np.float64))
    assert np.array_equal(model.narrow(w, dither), u)


def test_ordered_tile_means_are_exact_on_quarter_codes():
    """Every aligned 8 x 8 tile of a constant quarter code q / 4, q = 0..1020: the mean of the 64 results is exactly q / 4."""
    q = np.arange(1021)
    frames = np.broadcast_to((q / 4.0).astype(np.float16)[:, None, None, None], (1021, 16, 24, 3))
    assert np.array_equal(frames[:, 0, 0, 0].astype(np.float64) * 4, q)        # every quarter code is a half
    out = model.narrow(frames, "ordered").astype(np.int64)
    tiles = out.reshape(1021, 2, 8, 3, 8, 3).sum(axis=(2, 4))                 # [q, tile row, tile column, channel]
    assert np.array_equal(tiles, np.broadcast_to((16 * q)[:, None, None, None], tiles.shape))      # 64 * q / 4


def test_half_codes_ordered_against_none():
    k = np.arange(255)
    frames = np.broadcast_to((k + 0.5).astype(np.float16)[:, None, None, None], (255, 16, 8, 3))
    none, o = model.narrow(frames, "none"), model.narrow(frames, "ordered")
    assert np.array_equal(none[:, 0, 0, 0], k + (k & 1))                       # ties to even
    assert (none == none[:, :1, :1, :1]).all()
    diff = (none != o)
    assert (diff.reshape(255, -1).sum(axis=1) == 16 * 8 * 3 // 2).all()        # exactly half the pixels of every frame
    assert np.array_equal(o, k[:, None, None, None] + np.broadcast_to((model.BAYER8 >= 32)[None, np.arange(16) & 7][..., None], o.shape))


@pytest.mark.parametrize("dither", model.DITHERS)
def test_grey_in_gives_grey_out(dither):
    rng = np.random.default_rng(31)
    grey = (rng.random((2, 19, 27, 1), dtype=np.float32) * 300 - 20).astype(np.float16)
    out = model.narrow(np.broadcast_to(grey, (2, 19, 27, 3)), dither)
    assert (out == out[..., :1]).all()


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------------------

_vp = ctypes.c_void_p
SIGNATURES = {
    "crtfx_depth_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_vp)]),
    "crtfx_depth_destroy": (ctypes.c_int, [_vp]),
    "crtfx_depth_last_error": (ctypes.c_char_p, [_vp]),
    "crtfx_depth_run": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_int, _vp]),
    "crtfx_depth_set_option": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "crtfx_depth_last_plan": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_size_t]),
}


def test_symbols_are_bound_and_the_header_declares_them():
    assert _lib.DEPTH_SYMBOLS == SIGNATURES and _lib.DEPTH_OPT_FORCE_GENERAL == 1
    assert (_lib.DEPTH_WIDEN, _lib.DEPTH_NARROW, _lib.DITHER_NONE, _lib.DITHER_ORDERED) == (0, 1, 0, 1)
    lib = _lib.load()
    for name, (res, args) in SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res, name
    hdr = open(HEADER).read()
    for text in ("CRTFX_DEPTH_OPT_FORCE_GENERAL = 1", "CRTFX_DEPTH_WIDEN = 0", "CRTFX_DEPTH_NARROW = 1", "CRTFX_DITHER_NONE = 0", "CRTFX_DITHER_ORDERED = 1"):
        assert text in hdr, text
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(crtfx_depth_\w+)\s*\(([^)]*)\)\s*;", hdr)}
    assert set(protos) == set(SIGNATURES) and len(protos) == 6, set(protos) ^ set(SIGNATURES)
    for name, args in protos.items():
        assert len(args.split(",")) == len(SIGNATURES[name][1]), name
    order = [a.split()[-1].lstrip("*") for a in protos["crtfx_depth_create"].split(",")]
    assert order == ["device", "h", "w", "direction", "dither", "out_plan"]
    others = set()
    for table in ("SYMBOLS", "INGEST_SYMBOLS", "EGRESS_SYMBOLS", "UNPACK_SYMBOLS", "DEEP_SYMBOLS", "YUV422_SYMBOLS", "DEEP444_SYMBOLS", "SITED_SYMBOLS",
                  "EGRESS_SITED_SYMBOLS", "RESIZE16_SYMBOLS", "RESAMPLE_SYMBOLS", "CANVAS_SYMBOLS"):
        others |= set(getattr(_lib, table))
    assert not set(SIGNATURES) & others
    assert all(os.path.basename(f) in {os.path.basename(s) for s in _lib.SOURCES} for f in ("crtfx_depth.hip", "crtfx_depth.h"))
    assert all(os.path.exists(s) for s in _lib.SOURCES) and "crtfx_depth" in _lib.STAGE_UNITS
    import pythoncrt_amd as pc
    assert pc.Widen is depth.Widen and pc.Narrow is depth.Narrow and "Widen" in pc.__all__ and "Narrow" in pc.__all__
    assert issubclass(pc.Widen, _stage.Handle) and issubclass(pc.Narrow, _stage.Handle)
    import bench                                                               # a namespace of its own, outside the chain's evidence hash
    assert "crtfx_depth" not in open(bench.__file__).read()
    assert "namespace crtfx_depth_impl" in open(os.path.join(_lib.CSRC, "crtfx_depth.hip")).read()


GOOD = dict(device=0, h=9, w=24, direction=_lib.DEPTH_NARROW, dither=_lib.DITHER_ORDERED)


def _create(lib, no_out=False, **kw):
    a = dict(GOOD)
    a.update(kw)
    plan = ctypes.c_void_p(1)
    rc = lib.crtfx_depth_create(*(a[k] for k in GOOD), None if no_out else ctypes.byref(plan))
    return rc, plan, (lib.crtfx_depth_last_error(None) or b"").decode()


def test_create_refuses_bad_arguments_before_it_touches_a_device():
    """Every refusal of crtfx_depth_create comes before the device is asked for, so it holds on any machine; *out_plan is NULL and the
    message names the offending field."""
    lib = _lib.load()
    cases = [({k: v}, k + " =") for k in ("h", "w") for v in (0, -3, 32768)]
    cases += [(dict(direction=2), "direction"), (dict(direction=-1), "direction"), (dict(dither=2), "dither"), (dict(dither=-1), "dither"),
              (dict(direction=_lib.DEPTH_WIDEN, dither=_lib.DITHER_ORDERED), "dither")]
    for kw, word in cases:
        rc, plan, msg = _create(lib, **kw)
        assert rc == _lib.E_INVALID and not plan.value and word in msg, (kw, rc, plan.value, msg)
    rc, plan, msg = _create(lib, direction=_lib.DEPTH_WIDEN, dither=_lib.DITHER_ORDERED)
    assert "widen" in msg
    rc, plan, msg = _create(lib, no_out=True)
    assert rc == _lib.E_INVALID and "out_plan" in msg
    import torch
    if not torch.cuda.is_available():                                          # what is admitted passes every check: what is left to fail is the device
        for kw in (dict(), dict(dither=_lib.DITHER_NONE), dict(direction=_lib.DEPTH_WIDEN, dither=_lib.DITHER_NONE), dict(h=1, w=1), dict(h=32767, w=32767)):
            rc, plan, msg = _create(lib, **kw)
            assert rc == _lib.E_HIP and not plan.value and "device" in msg.lower(), (kw, rc, msg)
    else:
        rc, plan, msg = _create(lib, device=4096)
        assert rc == _lib.E_HIP and not plan.value and "4096" in msg
    assert lib.crtfx_depth_destroy(None) == _lib.OK and lib.crtfx_depth_set_option(None, 1, 1) == _lib.E_INVALID
    assert lib.crtfx_depth_run(None, None, 0, None, 0, 1, None) == _lib.E_INVALID
    assert lib.crtfx_depth_last_plan(None, ctypes.create_string_buffer(8), 8) == _lib.E_INVALID


def test_python_plans_refuse_before_a_device():
    with pytest.raises(ValueError, match="ROCm device"):
        depth.Widen("cpu", (4, 4))
    with pytest.raises(ValueError, match="ROCm device"):
        depth.Narrow("cpu", (4, 4))
    with pytest.raises(ValueError, match="dither"):
        depth.Narrow("cpu", (4, 4), dither="bayer")


# what include/crtfx_depth.h states for the six builds: VGPRs as built
HEADER_VGPRS = {"k_narrow<none,vec>": 24, "k_narrow<ordered,vec>": 36, "k_narrow<none,general>": 4, "k_narrow<ordered,general>": 7,
                "k_widen<vec>": 22, "k_widen<general>": 4}


def test_depth_kernels_hold_the_register_budget_and_the_header():
    """Registers, LDS and scratch of the six builds, read from the built library's code objects (tools/kernel_resources.py): at most 64
    VGPRs + AGPRs, no LDS, no scratch memory, no spills — and the figures the header quotes are the figures of this build."""
    import kernel_resources
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    res = kernel_resources.resources(_lib.LIB_PATH)
    found = {n.replace("crtfx_depth_impl::", "").replace(", ", ","): v for n, v in res.items() if n.startswith("crtfx_depth_impl::")}
    assert set(found) == set(HEADER_VGPRS), sorted(found)
    hdr = open(HEADER).read()
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
    for bad in ("uint8", "", None, "HALF", 16):
        with pytest.raises(ValueError, match="chain_pix.*dither"):
            run(chain_pix=bad)
    for bad in ("bayer", "", None, "ORDERED", True):
        for chain in ("auto", "half"):
            with pytest.raises(ValueError, match="dither.*chain_pix"):
                run(dither=bad, chain_pix=chain)
    # a dither where no Narrow would stand: the uint8 or 10-bit chain of "auto", a 10-bit delivery
    for kw in (dict(), dict(chain_pix="auto"), dict(chain_pix="auto", out_pix_fmt="nv12"), dict(in_pix_fmt="p010le", out_pix_fmt="p010le"),
               dict(chain_pix="half", in_pix_fmt="p010le", out_pix_fmt="p010le"), dict(chain_pix="half", out_pix_fmt="x2rgb10le"),
               dict(chain_pix="half", in_pix_fmt="nv12", out_pix_fmt="yuv420p10le")):
        with pytest.raises(ValueError, match="dither='ordered' with chain_pix="):
            run(dither="ordered", **kw)
    # "auto" is the code as it was: one 10-bit end is refused in the words it always was
    for kw in (dict(in_pix_fmt="p010le"), dict(out_pix_fmt="x2rgb10le"), dict(in_pix_fmt="nv12", out_pix_fmt="yuv420p10le", chain_pix="auto")):
        with pytest.raises(ValueError, match="a 10-bit format on one end only — the chain between them runs on half pixels or on uint8 ones"):
            run(**kw)
    # "half" admits them: the next thing asked for is the device
    for kw in (dict(in_pix_fmt="p010le"), dict(out_pix_fmt="x2rgb10le"), dict(in_pix_fmt="nv12", out_pix_fmt="yuv420p10le"), dict(),
               dict(dither="ordered"), dict(in_pix_fmt="p010le", out_pix_fmt="yuv420p", dither="ordered"),
               dict(in_pix_fmt="nv12", in_size=(50, 90), out_pix_fmt="yuv420p10le"), dict(resize_on="host")):
        with pytest.raises(AssertionError, match="the device was asked for"):
            run(chain_pix="half", **kw)
    # ... and a 10-bit source keeps its refusals under it
    with pytest.raises(ValueError, match=r"in_size=\(50, 90\) differs from the output size \(46, 80\): a 10-bit input cannot be resized"):
        run(chain_pix="half", in_pix_fmt="p010le", in_size=(50, 90))
    with pytest.raises(ValueError, match="in_crop.*cannot be resized"):
        run(chain_pix="half", in_pix_fmt="p010le", out_pix_fmt="nv12", in_crop=(0, 0, 40, 80))
    with pytest.raises(ValueError, match="resize_on='host' cannot be combined with in_pix_fmt"):
        run(chain_pix="half", in_pix_fmt="nv12", resize_on="host")


def test_cli_flags_refusals_and_the_sharded_cli(tmp_path, monkeypatch):
    from pythoncrt_amd import cli
    src = tmp_path / "in.rgb"
    src.write_bytes(bytes(46 * 80 * 3))
    out = tmp_path / "out.rgb"
    base = ["--input", str(src), "--output", str(out), "--width", "80", "--height", "46"]

    def refused(extra, *words):
        with pytest.raises(SystemExit) as e:
            cli.main(base + extra)
        assert e.value.code not in (0, None) and all(w in str(e.value) for w in words), (extra, str(e.value))
        assert not out.exists()
    for extra in ([], ["--chain-pix", "auto"], ["--out-pix-fmt", "nv12"], ["--in-pix-fmt", "p010le", "--out-pix-fmt", "p010le"],
                  ["--chain-pix", "half", "--in-pix-fmt", "p010le", "--out-pix-fmt", "p010le"], ["--chain-pix", "half", "--out-pix-fmt", "x2rgb10le"]):
        refused(["--dither", "ordered"] + extra, "--dither ordered", "--chain-pix")
    refused(["--in-pix-fmt", "p010le"], "a 10-bit format on one end only")       # "auto": as it was
    refused(["--out-pix-fmt", "yuv420p10le", "--chain-pix", "auto"], "a 10-bit format on one end only")
    refused(["--chain-pix", "half", "--in-pix-fmt", "p010le", "--in-crop-width", "40", "--in-crop-height", "46"], "--in-crop-width", "cannot be resized")
    for extra in (["--chain-pix", "uint8"], ["--dither", "bayer"], ["--chain-pix"], ["--dither"]):      # argparse's own refusal of an unknown choice
        with pytest.raises(SystemExit):
            cli.main(base + extra)
    # the two flags live in add_output_flags, not in the reference's schema
    assert not any(act.dest in ("chain_pix", "dither") for act in cli.build_parser()._actions)
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ["--chain-pix", "half"])
    a = cli.add_output_flags(cli.build_parser()).parse_args(base)
    assert (a.chain_pix, a.dither) == ("auto", "none")
    a = cli.add_input_flags(cli.add_output_flags(cli.build_parser())).parse_args(base + ["--chain-pix", "half", "--dither", "ordered", "--in-pix-fmt", "p010le"])
    assert (a.chain_pix, a.dither) == ("half", "ordered")
    spec, ranks = cli.check_flags(a)
    assert spec.deliver is None and spec.half is True and ranks is None        # admitted: delivered as rendered, a half chain, one process
    a = cli.add_input_flags(cli.add_output_flags(cli.build_parser())).parse_args(base)
    spec, ranks = cli.check_flags(a)
    assert spec.deliver is None and spec.half is False and ranks is None
    monkeypatch.setenv("CRTFX_FORCE_DIST", "1")
    refused(["--chain-pix", "half"], "sharded CLI", "--chain-pix half", "--dither")
    refused(["--chain-pix", "half", "--dither", "ordered"], "sharded CLI", "--chain-pix half", "--dither")
    refused(["--dither", "ordered"], "--dither ordered", "--chain-pix")


# ---- which stages the chain ends build --------------------------------------------------------------------------------------------------------

RESIZES = (ingest.IngestResize, resize16.ResizeHalf, resample.Resample)
FORMAT_PLANS = sorted({f.source for f in formats.FORMATS.values()} | {f.egress for f in formats.FORMATS.values()}, key=lambda c: c.__name__)


@pytest.fixture
def built(monkeypatch):
    """Every plan class records (class name, positional arguments past the device, keywords) instead of creating its plan; a format plan
    still knows its frame_bytes, as StagePlan.__init__ sets it."""
    log = []
    for cls in list(RESIZES) + FORMAT_PLANS + [canvas.Canvas, depth.Widen, depth.Narrow]:
        def init(self, *args, _cls=cls, **kw):
            log.append((_cls.__name__, args[1:], kw))
            if issubclass(_cls, _stage.StagePlan):
                self.frame_bytes = _cls._frame_bytes(args[1][0], args[1][1], kw["layout"])
        monkeypatch.setattr(cls, "__init__", init)
    return log


R, S, D = (24, 32), (48, 64), (12, 16)              # render, an off-size source, a delivery
NV12 = {"layout": "nv12", "matrix": "bt601", "range": "tv"}
P010 = {"layout": "p010le", "matrix": "bt601", "range": "tv"}
I420 = {"layout": "yuv420p", "matrix": "bt601", "range": "tv"}
X2 = {"layout": "x2rgb10le", "matrix": "bt601", "range": "tv"}
# source format -> chain_pix -> what SourceEnd builds for a source of size S (R for p010le: a 10-bit source is not resized), in order
SOURCE_TABLE = {
    ("rgb24", "auto"): [("IngestResize", (S, R), {})],
    ("rgb24", "half"): [("IngestResize", (S, R), {}), ("Widen", (R,), {})],
    ("nv12", "auto"): [("UnpackYuv", (S,), NV12), ("IngestResize", (S, R), {})],
    ("nv12", "half"): [("UnpackYuv", (S,), NV12), ("IngestResize", (S, R), {}), ("Widen", (R,), {})],
    ("p010le", "auto"): [("UnpackYuv10", (R,), P010)],
    ("p010le", "half"): [("UnpackYuv10", (R,), P010)],
}
# delivery format -> chain_pix -> what DeliveryEnd builds for a delivery of size D under dither "ordered" where one is allowed
DELIVERY_TABLE = {
    ("rgb24", "auto"): [("IngestResize", (R, D), {})],
    ("rgb24", "half"): [("ResizeHalf", (R, D), {}), ("Narrow", (D,), {"dither": "ordered"})],
    ("yuv420p", "auto"): [("IngestResize", (R, D), {}), ("EgressYuv", (D,), I420)],
    ("yuv420p", "half"): [("ResizeHalf", (R, D), {}), ("Narrow", (D,), {"dither": "ordered"}), ("EgressYuv", (D,), I420)],
    ("x2rgb10le", "auto"): [("ResizeHalf", (R, D), {}), ("EgressDeep444", (D,), X2)],
    ("x2rgb10le", "half"): [("ResizeHalf", (R, D), {}), ("EgressDeep444", (D,), X2)],
}


@pytest.mark.parametrize("chain", ["auto", "half"])
@pytest.mark.parametrize("out_fmt", ["rgb24", "yuv420p", "x2rgb10le"])
@pytest.mark.parametrize("in_fmt", ["rgb24", "nv12", "p010le"])
def test_chain_end_stage_lists(built, monkeypatch, in_fmt, out_fmt, chain):
    import torch
    deep_in, deep_out = in_fmt == "p010le", out_fmt == "x2rgb10le"
    if chain == "auto" and deep_in != deep_out:                                # refused, as it always was: there are no ends to build
        run = _refusing_process_frames(monkeypatch)
        with pytest.raises(ValueError, match="a 10-bit format on one end only"):
            run(in_pix_fmt=in_fmt, out_pix_fmt=out_fmt, chain_pix=chain)
        return
    dither = "ordered" if chain == "half" and not deep_out else "none"
    half, widen, narrow = ends.depth_stages(in_fmt, out_fmt, chain, dither)
    assert half == (chain == "half" or (deep_in and deep_out))
    assert widen == (chain == "half" and not deep_in) and narrow == ("ordered" if chain == "half" and not deep_out else None)
    pix = torch.float16 if half else torch.uint8
    src_hw = R if deep_in else S
    src = ends.SourceEnd("dev", R, in_fmt, "bt601", "tv", "replicate", src_hw, "bilinear", None, pix, widen=widen)
    assert built == SOURCE_TABLE[(in_fmt, chain)], built
    assert [type(st).__name__ for st, _ in src.stages] == [b[0] for b in built]
    assert [hw for _, hw in src.stages] == [b[1][-1] for b in built]         # each stage's frames have the last size it was built with
    assert src.dtype == (torch.float16 if deep_in else torch.uint8) and (src.widen is not None) == widen
    del built[:]
    end = ends.DeliveryEnd("dev", R, pix, out_fmt, "bt601", "tv", "center", D, "bilinear", narrow=narrow)
    assert built == DELIVERY_TABLE[(out_fmt, chain)], built
    front = [b for b in built if not b[0].startswith("Egress")]
    assert [type(st).__name__ for st, _ in end.stages] == [b[0] for b in front] and [hw for _, hw in end.stages] == [D] * len(front)
    assert (end.narrow is not None) == (narrow is not None) and (end.egress is None) == (out_fmt == "rgb24")
    assert end.size == D and end.frame_bytes == formats.frame_bytes(D[0], D[1], out_fmt)


def test_the_default_arguments_build_todays_lists(built):
    """Without the new parameters — and with an rgb24 frame at render size under them — the ends build what they built, and what the depth
    stage adds: nothing for the defaults, one Widen / one Narrow as the only stage."""
    import torch
    u8, f16 = torch.uint8, torch.float16
    src = ends.SourceEnd("dev", R, "rgb24", "bt601", "tv", "replicate", R, "bilinear")
    assert built == [] and src.stages == [] and src.widen is None and src.dtype == u8
    src = ends.SourceEnd("dev", R, "nv12", "bt601", "tv", "replicate", S, "bicubic", (6, 0, 36, 64))
    assert [b[0] for b in built] == ["UnpackYuv", "Canvas", "Resample"] and src.widen is None
    del built[:]
    end = ends.DeliveryEnd("dev", R, u8, "rgb24", "bt601", "tv", "center", None, "bilinear")
    assert built == [] and end.stages == [] and end.narrow is None and end.shape(3) == (3,) + R + (3,)
    end = ends.DeliveryEnd("dev", R, f16, "p010le", "bt601", "tv", "center", D, "lanczos", "stretch", (0, 0, 0))
    assert [b[0] for b in built] == ["Resample", "EgressYuv10"] and end.narrow is None
    del built[:]
    assert ends.depth_stages("rgb24", "rgb24") == (False, False, None) and ends.depth_stages("p010le", "x2rgb10le") == (True, False, None)
    assert ends.depth_stages("p010le", "x2rgb10le", "half", "none") == (True, False, None)      # 10-bit on both ends: "half" builds no depth plan
    # rgb24 at render size under a half chain: a source end whose only stage is the Widen, a delivery whose only stage is the Narrow
    src = ends.SourceEnd("dev", R, "rgb24", "bt601", "tv", "replicate", R, "bilinear", None, f16, widen=True)
    assert built == [("Widen", (R,), {})] and [hw for _, hw in src.stages] == [R] and src.frame_shape == R + (3,) and src.dtype == u8
    del built[:]
    end = ends.DeliveryEnd("dev", R, f16, "rgb24", "bt601", "tv", "center", None, "bilinear", narrow="none")
    assert built == [("Narrow", (R,), {"dither": "none"})] and [hw for _, hw in end.stages] == [R] and end.shape(3) == (3,) + R + (3,)
    # the Narrow stands behind the half geometry, at the delivery size
    del built[:]
    end = ends.DeliveryEnd("dev", (48, 64), f16, "nv12", "bt601", "tv", "center", (36, 64), "bilinear", deliver_fit="pad", pad_color=(7, 200, 33),
                           narrow="ordered")
    assert built == [("ResizeHalf", ((48, 64), (36, 48)), {}), ("Canvas", ((36, 48), (36, 64)), {"at": (0, 8), "fill": (7, 200, 33), "dtype": f16}),
                     ("Narrow", ((36, 64),), {"dither": "ordered"}), ("EgressYuv", ((36, 64),), {"layout": "nv12", "matrix": "bt601", "range": "tv"})]
