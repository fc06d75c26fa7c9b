"""The filtered resampler on the GPU: Resample (k_resample_fused, and k_resample_h + k_resample_v) under all five filters — uint8 frames against
Pillow itself, zero differing bytes; half frames against the int64 model (tests/resample_model.py, which tests/test_resample_tables.py holds
to the installed Pillow), zero differing elements on the uint16 view."""
import ctypes

import numpy as np
import pytest

from pythoncrt_amd import _lib
from tests import pil_resize_model, resize16_model
from tests import resample_model as model

pytestmark = pytest.mark.gpu

FUSED, GENERAL = "k_resample_fused<", "k_resample_h+k_resample_v<"
FAR = ((360, 640), (9, 16))            # a 1/40 reduction: no tile fits the LDS budget under any filter but box
# which pair reaches which tile shape of the fused path under bicubic (rows / cols clipped to the output size), in the order of the planner's list
SHAPE_PAIRS = {
    "u8": [(((48, 64), (96, 128)), "rows=32,cols=128"), (((40, 200), (20, 130)), "rows=20,cols=64"), (((108, 192), (54, 96)), "rows=16,cols=96"),
           (((64, 300), (33, 140)), "rows=16,cols=64"), (((100, 300), (34, 100)), "rows=8,cols=64"), (((80, 400), (20, 100)), "rows=8,cols=32"),
           (((40, 330), (9, 40)), "rows=4,cols=32")],
    "half": [(((48, 64), (96, 128)), "rows=32,cols=128"), (((120, 213), (119, 214)), "rows=32,cols=64"), (((100, 25), (40, 100)), "rows=16,cols=100"),
             (((40, 200), (20, 130)), "rows=16,cols=64"), (((108, 192), (54, 96)), "rows=8,cols=64"), (((70, 200), (34, 66)), "rows=8,cols=32"),
             (((20, 330), (8, 40)), "rows=4,cols=32")]}
BASE_PAIRS = pil_resize_model.PAIRS + pil_resize_model.EXTRA_PAIRS
SHAPE_ONLY = sorted({p for px in SHAPE_PAIRS for p, _ in SHAPE_PAIRS[px] if p not in BASE_PAIRS})
CASES = [(f, p) for f in model.FILTERS for p in BASE_PAIRS] + [("bicubic", p) for p in SHAPE_ONLY]


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _torch_dtype(px):
    import torch
    return torch.uint8 if px == "u8" else torch.float16


def _bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.uint8 else a.view(np.uint16)


def _to_dev(frames_np):
    """Frames with their bit patterns kept (the NaN payloads of half frames included): halves are moved as int16."""
    import torch
    if frames_np.dtype == np.uint8:
        return torch.from_numpy(np.ascontiguousarray(frames_np)).to(_dev())
    return torch.from_numpy(_bits(frames_np).view(np.int16)).to(_dev()).view(torch.float16)


def _to_host(t):
    import torch
    return t.cpu().numpy() if t.dtype == torch.uint8 else t.view(torch.int16).cpu().numpy().view(np.float16)


def _resize(src_np, dst, filter, force_general=False, acc64=False):
    """(the frames from the device, the plan dictionary) for a stack of equal-size frames."""
    import torch
    from pythoncrt_amd import Resample
    plan = Resample(_dev(), src_np.shape[1:3], dst, filter=filter, dtype=_torch_dtype("u8" if src_np.dtype == np.uint8 else "half"))
    if force_general:
        plan.set_option(_lib.RESAMPLE_OPT_FORCE_GENERAL, 1)
    if acc64:
        plan.set_option(_lib.RESAMPLE_OPT_ACC64, 1)
    out = plan.run(_to_dev(src_np))
    torch.cuda.synchronize()
    got, how = _to_host(out), plan.plan()
    plan.close()
    return got, how


_EXPECTED = {}


def _case(px, filter, src, dst):
    """(the two test images as one batch, the expected result): computed once per case, shared by both paths.  uint8: Pillow itself; half:
    the model."""
    key = (px, filter, src, dst)
    if key not in _EXPECTED:
        if px == "u8":
            imgs = pil_resize_model.images(*src)
            frames = np.stack([imgs["random"], imgs["binary"]])
            exp = np.stack([model.pillow(f, dst[0], dst[1], filter) for f in frames])
        else:
            imgs = resize16_model.images(*src)
            frames = np.stack([imgs["random"], imgs["binary"]])
            exp = model.resize_half(frames, dst[0], dst[1], filter)
        exp.setflags(write=False)
        _EXPECTED[key] = (frames, exp)
    return _EXPECTED[key]


def _fits(px, filter, src, dst):
    return model.fused_shape(src, dst, filter, 1 if px == "u8" else 2)


@pytest.mark.parametrize("force_general", [False, True], ids=["default", "general"])
@pytest.mark.parametrize("filter,pair", CASES, ids=lambda v: v if isinstance(v, str) else f"{v[0][0]}x{v[0][1]}-{v[1][0]}x{v[1][1]}")
@pytest.mark.parametrize("px", ["u8", "half"])
def test_resize_equals_pillow_and_the_model(px, filter, pair, force_general):
    """Every filter x every pair of the 8-bit resampler's lists (up, down, ragged, degenerate, the 1/40 reduction, row starts on every byte
    offset mod 4), plus the pairs that reach the remaining tile shapes; the random image (halves: the whole range of the format, NaN, +-inf
    and negatives included) and the 0 / 255 one — full-scale steps, which overshoot on both sides under bicubic and Lanczos — as one batch of
    two; both paths.  uint8 against Pillow's own bytes, half against the model's bit patterns: 0 differ; the plan names the path that ran
    and the tile shape and LDS bytes the header's formula gives."""
    src, dst = pair
    frames, exp = _case(px, filter, src, dst)
    got, how = _resize(frames, dst, filter, force_general)
    assert got.shape == exp.shape and got.dtype == exp.dtype
    bad = int((_bits(got) != _bits(exp)).sum())
    assert bad == 0, (px, filter, src, dst, how, bad)
    assert how["frames"] == "2"
    fits = _fits(px, filter, src, dst)
    if force_general or fits is None:
        assert how == {"resample": f"{GENERAL}{px}>", "frames": "2"}, how
    else:
        assert how == {"resample": f"{FUSED}{px},rows={fits[0]},cols={fits[1]}>", "lds": str(fits[2]), "frames": "2"}, how
    if pair == FAR and filter != "box":
        assert fits is None                                     # 241 taps per axis under Lanczos: the general path by default


@pytest.mark.parametrize("px", ["u8", "half"])
def test_every_tile_shape_is_reached_and_the_general_path_is_taken_by_default_somewhere(px):
    """plan() before the first run names the path the next run takes: each of the seven tile shapes for its pair of SHAPE_PAIRS under bicubic
    (all of them run in test_resize_equals_pillow_and_the_model), the general path for the 1/40 Lanczos reduction, and the header's figures
    for the full-size pairs."""
    from pythoncrt_amd import Resample
    dt = _torch_dtype(px)
    for (src, dst), shape in SHAPE_PAIRS[px]:
        p = Resample(_dev(), src, dst, filter="bicubic", dtype=dt)
        assert p.plan()["resample"] == f"{FUSED}{px},{shape}>" and p.plan()["frames"] == "0", (src, dst, p.plan())
        p.close()
    shapes = [tuple(int(v.split("=")[1]) for v in s.split(",")) for _, s in SHAPE_PAIRS[px]]
    # rows / cols are clipped to the output: each entry stands for one of the planner's seven, in its order
    planner = ((32, 128), (32, 64), (16, 128), (16, 64), (8, 64), (8, 32), (4, 32))
    assert len(shapes) == 7 and all(s[0] <= t[0] and s[1] <= t[1] and (i == 0 or s != shapes[i - 1]) for i, (s, t) in enumerate(zip(shapes, planner)))
    for (src, dst), shape in SHAPE_PAIRS[px]:
        i = [s for _, s in SHAPE_PAIRS[px]].index(shape)
        rows, cols = min(planner[i][0], dst[0]), min(planner[i][1], dst[1])
        assert shape == f"rows={rows},cols={cols}", (src, dst, shape)
    a = Resample(_dev(), FAR[0], FAR[1], filter="lanczos", dtype=dt)
    assert a.plan() == {"resample": f"{GENERAL}{px}>", "frames": "0"}, a.plan()
    a.close()
    UHD, FHD = (2160, 3840), (1080, 1920)
    for filter, src, dst, u8, half in (("lanczos", UHD, FHD, ("rows=16,cols=64", 30672), ("rows=8,cols=64", 36040)),
                                       ("lanczos", FHD, UHD, ("rows=32,cols=128", 19048), ("rows=32,cols=128", 32072)),
                                       ("bicubic", UHD, FHD, ("rows=16,cols=64", 26472), ("rows=8,cols=64", 29480)),
                                       ("lanczos", UHD, (540, 960), ("rows=8,cols=32", 32816), None)):
        want = u8 if px == "u8" else half
        p = Resample(_dev(), src, dst, filter=filter, dtype=dt)
        if want is None:
            assert p.plan() == {"resample": f"{GENERAL}{px}>", "frames": "0"}, p.plan()
        else:
            assert p.plan() == {"resample": f"{FUSED}{px},{want[0]}>", "lds": str(want[1]), "frames": "0"}, (filter, src, dst, p.plan())
        p.close()


@pytest.mark.parametrize("px", ["u8", "half"])
def test_bilinear_on_this_stage_is_the_bilinear_stage(px):
    """Resample(filter="bilinear") against IngestResize / ResizeHalf on the same input, both paths: the same bits."""
    import torch
    from pythoncrt_amd import IngestResize, ResizeHalf
    for src, dst in (((48, 64), (96, 128)), ((45, 80), (67, 123)), ((108, 192), (54, 96)), ((37, 63), (53, 87)), FAR):
        frames, _ = _case(px, "bilinear", src, dst)
        old = (IngestResize if px == "u8" else ResizeHalf)(_dev(), src, dst)
        ref = _to_host(old.run(_to_dev(frames)))
        torch.cuda.synchronize()
        old.close()
        for force in (False, True):
            got, how = _resize(frames, dst, "bilinear", force)
            assert np.array_equal(_bits(got), _bits(ref)), (px, src, dst, how)


def test_the_int64_accumulator_gives_the_same_bits():
    """CRTFX_RESAMPLE_OPT_ACC64: a 64-bit multiply-add per tap in place of the two int32 accumulators — the same elements on both paths; the
    plan says so; a uint8 plan refuses the option."""
    import torch
    from pythoncrt_amd import Resample
    from pythoncrt_amd._lib import CrtfxError
    for filter, (src, dst) in (("lanczos", ((108, 192), (54, 96))), ("bicubic", ((45, 80), (67, 123))), ("lanczos", ((37, 62), (53, 86))), ("lanczos", FAR)):
        frames, exp = _case("half", filter, src, dst)
        for force in (False, True):
            got, how = _resize(frames, dst, filter, force, acc64=True)
            assert how["acc"] == "i64" and (how["resample"].startswith(GENERAL) == (force or (src, dst) == FAR)), how
            assert int((_bits(got) != _bits(exp)).sum()) == 0, (filter, src, dst, how)
    p = Resample(_dev(), (8, 8), (16, 16), dtype=torch.uint8)
    with pytest.raises(CrtfxError) as e:
        p.set_option(_lib.RESAMPLE_OPT_ACC64, 1)
    assert e.value.code == _lib.E_INVALID and "half" in str(e.value)
    p.close()


@pytest.mark.parametrize("px", ["u8", "half"])
def test_strided_batches_leave_the_padding_alone(px):
    """n = 3 frames that are slices of bigger tensors on both sides (strides larger than a frame, bases on every offset of a dword): every
    frame right, every element in front of, between and behind the frames untouched — on both paths, Lanczos."""
    import torch
    from pythoncrt_amd import Resample
    src, dst, n = (45, 80), (67, 123), 3
    rng = np.random.default_rng(3)
    if px == "u8":
        frames = rng.integers(0, 256, (n,) + src + (3,), dtype=np.uint8)
        exp = np.stack([model.pillow(f, dst[0], dst[1], "lanczos") for f in frames])
        raw, fill, guard = torch.uint8, 0xA5, 0x5A
    else:
        frames = (rng.random((n,) + src + (3,)) * 300.0 - 20.0).astype(np.float16)
        exp = model.resize_half(frames, dst[0], dst[1], "lanczos")
        raw, fill, guard = torch.int16, 0x7E00, 0x5A5A                                                  # NaN between the source frames
    dt = _torch_dtype(px)
    se, de = src[0] * src[1] * 3, dst[0] * dst[1] * 3
    for force in (0, 1):
        for s_off, d_off, s_pad, d_pad in ((1, 3, 7, 5), (2, 1, 64, 1), (3, 2, 2, 3), (0, 0, 0, 0)):
            sbuf = torch.full((s_off + n * (se + s_pad) + 16,), fill, dtype=raw, device=_dev())
            dbuf = torch.full((d_off + n * (de + d_pad) + 16,), guard, dtype=raw, device=_dev())
            sview = sbuf[s_off:s_off + n * (se + s_pad)].view(n, se + s_pad)[:, :se].unflatten(1, src + (3,)).view(dt)
            dview = dbuf[d_off:d_off + n * (de + d_pad)].view(n, de + d_pad)[:, :de].unflatten(1, dst + (3,)).view(dt)
            sview.copy_(_to_dev(frames))
            plan = Resample(_dev(), src, dst, filter="lanczos", dtype=dt)
            plan.set_option(_lib.RESAMPLE_OPT_FORCE_GENERAL, force)
            assert plan.run(sview, out=dview) is dview
            torch.cuda.synchronize()
            assert plan.plan()["frames"] == "3" and plan.plan()["resample"].startswith(GENERAL) == bool(force)
            got = _bits(_to_host(dview))
            assert np.array_equal(got, _bits(exp)), (px, force, s_off, d_off, int((got != _bits(exp)).sum()))
            keep = torch.ones_like(dbuf, dtype=torch.bool)
            keep[d_off:d_off + n * (de + d_pad)].view(n, de + d_pad)[:, :de] = False
            assert bool((dbuf[keep] == guard).all()), (px, force, s_off, d_off)
            plan.close()


def test_half_frames_on_odd_bytes_are_refused():
    import torch
    from pythoncrt_amd import Resample
    src, dst = (45, 80), (67, 123)
    se, de = src[0] * src[1] * 3, dst[0] * dst[1] * 3
    plan = Resample(_dev(), src, dst, dtype=torch.float16)
    a = torch.zeros((2 * se + 8,), dtype=torch.float16, device=_dev())
    b = torch.zeros((2 * de + 8,), dtype=torch.float16, device=_dev())
    st = torch.cuda.current_stream().cuda_stream
    for args in ((a.data_ptr() + 1, 2 * se, b.data_ptr(), 2 * de, 1), (a.data_ptr(), 2 * se, b.data_ptr() + 1, 2 * de, 1),
                 (a.data_ptr(), 2 * se + 1, b.data_ptr(), 2 * de, 2), (a.data_ptr(), 2 * se, b.data_ptr(), 2 * de + 1, 2)):
        assert plan.lib.crtfx_resample_run(plan._plan, args[0], args[1], args[2], args[3], args[4], st) == _lib.E_INVALID, args
        assert b"even" in plan.lib.crtfx_resample_last_error(plan._plan)
    torch.cuda.synchronize()
    assert bool((b == 0).all())
    plan.close()


@pytest.mark.parametrize("px", ["u8", "half"])
def test_a_4k_batch_of_two_to_1080p_lanczos(px):
    """2160 x 3840 -> 1080 x 1920 under Lanczos, two frames, the default (fused) path: the size a render is delivered at."""
    src, dst = (2160, 3840), (1080, 1920)
    frames, exp = _case(px, "lanczos", src, dst)
    got, how = _resize(frames, dst, "lanczos")
    want = {"u8": ("rows=16,cols=64", "30672"), "half": ("rows=8,cols=64", "36040")}[px]
    assert how == {"resample": f"{FUSED}{px},{want[0]}>", "lds": want[1], "frames": "2"}, how
    assert int((_bits(got) != _bits(exp)).sum()) == 0, int((_bits(got) != _bits(exp)).sum())


def test_bad_arguments_return_the_stated_codes():
    """A wrong dtype of the frames is UNSUPPORTED; a wrong shape, dtype of `out` or device is a ValueError; sizes < 1, bad options, n = 0,
    a null frame and short strides are INVALID; each leaves a message."""
    import torch
    from pythoncrt_amd import Resample
    from pythoncrt_amd._lib import CrtfxError
    with pytest.raises(CrtfxError) as e:
        Resample(_dev(), (8, 8), (0, 16))
    assert e.value.code == _lib.E_INVALID
    with pytest.raises(ValueError):
        Resample("cpu", (8, 8), (16, 16))
    with pytest.raises(ValueError, match="filter"):
        Resample(_dev(), (8, 8), (16, 16), filter="nearest")
    with pytest.raises(ValueError, match="dtype"):
        Resample(_dev(), (8, 8), (16, 16), dtype=torch.float32)
    for dt, other, item in ((torch.uint8, torch.float16, 1), (torch.float16, torch.uint8, 2)):
        plan = Resample(_dev(), (8, 8), (16, 16), dtype=dt)
        assert plan.filter == "lanczos" and plan.dtype == dt
        with pytest.raises(CrtfxError) as e:
            plan.run(torch.zeros((1, 8, 8, 3), dtype=other, device=_dev()))
        assert e.value.code == _lib.E_UNSUPPORTED
        with pytest.raises(ValueError):
            plan.run(torch.zeros((1, 8, 9, 3), dtype=dt, device=_dev()))
        with pytest.raises(ValueError):
            plan.run(torch.zeros((1, 8, 8, 3), dtype=dt))                                              # a host tensor
        with pytest.raises(ValueError):
            plan.run(torch.zeros((1, 8, 8, 3), dtype=dt, device=_dev()), out=torch.zeros((1, 16, 16, 3), dtype=other, device=_dev()))
        with pytest.raises(ValueError):
            plan.run(torch.zeros((1, 8, 3, 8), dtype=dt, device=_dev()).transpose(2, 3))                # frames that are not contiguous
        assert tuple(plan.run(torch.zeros((0, 8, 8, 3), dtype=dt, device=_dev())).shape) == (0, 16, 16, 3)
        with pytest.raises(CrtfxError) as e:
            plan.set_option(99, 1)
        assert e.value.code == _lib.E_INVALID and "option" in str(e.value)
        with pytest.raises(CrtfxError) as e:
            plan.set_option(_lib.RESAMPLE_OPT_FORCE_GENERAL, 2)
        assert e.value.code == _lib.E_INVALID
        lib = plan.lib
        src = torch.zeros((1, 8, 8, 3), dtype=dt, device=_dev())
        out = torch.zeros((1, 16, 16, 3), dtype=dt, device=_dev())
        st = torch.cuda.current_stream().cuda_stream
        sb, db = 192 * item, 768 * item
        assert lib.crtfx_resample_run(plan._plan, src.data_ptr(), sb, out.data_ptr(), db, 0, st) == _lib.E_INVALID
        assert b"n = 0" in lib.crtfx_resample_last_error(plan._plan)
        assert lib.crtfx_resample_run(plan._plan, None, sb, out.data_ptr(), db, 1, st) == _lib.E_INVALID
        assert lib.crtfx_resample_run(plan._plan, src.data_ptr(), sb - 2, out.data_ptr(), db, 2, st) == _lib.E_INVALID
        assert b"strides" in lib.crtfx_resample_last_error(plan._plan)
        if torch.cuda.device_count() > 1:
            with torch.cuda.device(1):
                assert lib.crtfx_resample_run(plan._plan, src.data_ptr(), sb, out.data_ptr(), db, 1, None) == _lib.E_INVALID
                assert b"current device" in lib.crtfx_resample_last_error(plan._plan)
        buf = ctypes.create_string_buffer(10)
        assert lib.crtfx_resample_last_plan(plan._plan, buf, 10) == _lib.OK and buf.value == b"resample="    # truncated, NUL-terminated
        plan.close()
        plan.close()
