"""The half resampler on the GPU: ResizeHalf (k_resize16_fused, and k_resize16_h + k_resize16_v) against the int64 model
(tests/resize16_model.py, which tests/test_resize16_tables.py ties to the installed Pillow) — zero differing elements on the uint16 view."""
import ctypes

import numpy as np
import pytest

from pythoncrt_amd import _lib
from tests import pil_resize_model
from tests import resize16_model as model

pytestmark = pytest.mark.gpu

FUSED, GENERAL = "k_resize16_fused<", "k_resize16_h+k_resize16_v"
# which pair reaches which tile shape of the fused path (rows / cols clipped to the output size), in the order of the planner's list
SHAPE_PAIRS = [(((48, 64), (96, 128)), "rows=32,cols=128"), (((120, 213), (119, 214)), "rows=32,cols=64"), (((100, 25), (40, 100)), "rows=16,cols=100"),
               (((40, 200), (20, 130)), "rows=16,cols=64"), (((108, 192), (54, 96)), "rows=8,cols=64"), (((20, 330), (8, 40)), "rows=8,cols=32"),
               (((20, 330), (8, 33)), "rows=4,cols=32")]
ALL_PAIRS = pil_resize_model.PAIRS + pil_resize_model.EXTRA_PAIRS + [p for p, _ in SHAPE_PAIRS if p not in pil_resize_model.PAIRS]


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _to_dev(frames_np):
    """float16 frames with their bit patterns kept (NaN payloads included): moved as int16."""
    import torch
    return torch.from_numpy(_bits(frames_np).view(np.int16)).to(_dev()).view(torch.float16)


def _resize(src_np, dst, force_general=False):
    """(float16[n, h, w, 3] from the device, the plan string) for a stack of equal-size frames."""
    import torch
    from pythoncrt_amd import ResizeHalf
    plan = ResizeHalf(_dev(), src_np.shape[1:3], dst)
    if force_general:
        plan.set_option(_lib.RESIZE16_OPT_FORCE_GENERAL, 1)
    out = plan.run(_to_dev(src_np))
    torch.cuda.synchronize()
    got, how = out.view(torch.int16).cpu().numpy().view(np.float16), plan.plan()
    plan.close()
    return got, how


_EXPECTED = {}


def _case(src, dst):
    """(the two test images as one batch, the model's result): computed once per pair, shared by both paths."""
    if (src, dst) not in _EXPECTED:
        imgs = model.images(*src)
        frames = np.stack([imgs["random"], imgs["binary"]])
        exp = model.resize(frames, *dst)
        exp.setflags(write=False)
        _EXPECTED[(src, dst)] = (frames, exp)
    return _EXPECTED[(src, dst)]


@pytest.mark.parametrize("force_general", [False, True], ids=["default", "general"])
@pytest.mark.parametrize("src,dst", ALL_PAIRS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_resize_equals_the_model(src, dst, force_general):
    """Every pair of the 8-bit resampler's lists (up, down, ragged, degenerate, the 1/40 reduction, row starts on either half of a dword)
    plus the pairs that reach the remaining tile shapes; a random image over the whole range of half (negatives, values above 255, NaN,
    +-inf) and a 0 / 255.0 one as one batch of two; both paths; 0 elements differ on the uint16 view; the plan names the path that ran."""
    frames, exp = _case(src, dst)
    assert np.isnan(frames[0].astype(np.float32)).any() or frames[0].size < 40
    got, how = _resize(frames, dst, force_general)
    assert got.shape == exp.shape and got.dtype == np.float16
    assert int((_bits(got) != _bits(exp)).sum()) == 0, (src, dst, how, int((_bits(got) != _bits(exp)).sum()))
    assert how["frames"] == "2"
    if force_general:
        assert how["resize16"] == GENERAL, how
    elif (src, dst) == ((360, 640), (9, 16)):
        assert how["resize16"] == GENERAL, how                 # 81 taps per axis: no tile fits the LDS budget
    else:
        assert how["resize16"].startswith(FUSED) and 0 < int(how["lds"]) <= 40960, how


def test_every_tile_shape_is_reached_and_the_general_path_is_taken_by_default_somewhere():
    """plan() before the first run names the path the next run takes: each of the seven tile shapes for its pair of SHAPE_PAIRS (all of them
    run in test_resize_equals_the_model), the general path for the 1/40 reduction, and the header's figures for the full-size pairs."""
    from pythoncrt_amd import ResizeHalf
    for (src, dst), shape in SHAPE_PAIRS:
        p = ResizeHalf(_dev(), src, dst)
        assert p.plan()["resize16"] == f"k_resize16_fused<{shape}>" and p.plan()["frames"] == "0", (src, dst, p.plan())
        p.close()
    assert len({s for _, s in SHAPE_PAIRS}) == 7
    a = ResizeHalf(_dev(), (360, 640), (9, 16))
    assert a.plan() == {"resize16": GENERAL, "frames": "0"}, a.plan()
    for src, dst, shape, lds in (((1080, 1920), (2160, 3840), "rows=32,cols=128", 24224), ((2160, 3840), (1080, 1920), "rows=8,cols=64", 23040),
                                 ((2160, 3840), (540, 960), "rows=8,cols=32", 37328)):
        p = ResizeHalf(_dev(), src, dst)
        assert p.plan() == {"resize16": f"k_resize16_fused<{shape}>", "lds": str(lds), "frames": "0"}, (src, dst, p.plan())
        p.close()


def test_strided_batches_leave_the_padding_alone():
    """n = 5 frames that are slices of bigger tensors on both sides (strides larger than a frame, bases on either half of a dword): every
    frame right, every element outside the frames untouched — on both paths.  Odd bases and odd strides are refused."""
    import torch
    from pythoncrt_amd import ResizeHalf
    src, dst, n = (45, 80), (67, 123), 5
    rng = np.random.default_rng(3)
    frames = (rng.random((n,) + src + (3,)) * 300.0 - 20.0).astype(np.float16)
    exp = model.resize(frames, *dst)
    se, de = src[0] * src[1] * 3, dst[0] * dst[1] * 3
    guard = np.array([0x5A5A], dtype=np.uint16).view(np.int16)[0]
    for force in (0, 1):
        for s_off, d_off, s_pad, d_pad in ((1, 3, 7, 5), (2, 1, 64, 1), (0, 0, 0, 0)):
            sbuf = torch.full((s_off + n * (se + s_pad) + 16,), 0x7E00, dtype=torch.int16, device=_dev())          # NaN between the source frames
            dbuf = torch.full((d_off + n * (de + d_pad) + 16,), int(guard), dtype=torch.int16, device=_dev())
            sview = sbuf[s_off:s_off + n * (se + s_pad)].view(n, se + s_pad)[:, :se].unflatten(1, src + (3,)).view(torch.float16)
            dview = dbuf[d_off:d_off + n * (de + d_pad)].view(n, de + d_pad)[:, :de].unflatten(1, dst + (3,)).view(torch.float16)
            sview.copy_(_to_dev(frames))
            plan = ResizeHalf(_dev(), src, dst)
            plan.set_option(_lib.RESIZE16_OPT_FORCE_GENERAL, force)
            assert plan.run(sview, out=dview) is dview
            torch.cuda.synchronize()
            assert plan.plan()["frames"] == "5" and (plan.plan()["resize16"] == GENERAL) == bool(force)
            got = dview.view(torch.int16).cpu().numpy().view(np.uint16)
            assert np.array_equal(got, _bits(exp)), (force, s_off, d_off, int((got != _bits(exp)).sum()))
            keep = torch.ones_like(dbuf, dtype=torch.bool)
            keep[d_off:d_off + n * (de + d_pad)].view(n, de + d_pad)[:, :de] = False
            assert bool((dbuf[keep] == int(guard)).all()), (force, s_off, d_off)
            plan.close()
    plan = ResizeHalf(_dev(), src, dst)
    a = torch.zeros((2 * se + 8,), dtype=torch.float16, device=_dev())
    b = torch.zeros((2 * de + 8,), dtype=torch.float16, device=_dev())
    st = torch.cuda.current_stream().cuda_stream
    for args in ((a.data_ptr() + 1, 2 * se, b.data_ptr(), 2 * de, 1), (a.data_ptr(), 2 * se, b.data_ptr() + 1, 2 * de, 1),
                 (a.data_ptr(), 2 * se + 1, b.data_ptr(), 2 * de, 2), (a.data_ptr(), 2 * se, b.data_ptr(), 2 * de + 1, 2)):
        assert plan.lib.crtfx_resize16_run(plan._plan, args[0], args[1], args[2], args[3], args[4], st) == _lib.E_INVALID, args
        assert b"even" in plan.lib.crtfx_resize16_last_error(plan._plan)
    torch.cuda.synchronize()
    assert bool((b == 0).all())
    plan.close()


def test_a_4k_batch_of_two_to_1080p():
    """2160 x 3840 -> 1080 x 1920, two frames, the default (fused) path: the size a render is delivered at.  The frames are the two test
    images of that size (resize16_model.images: halves over the whole range of the format, and the 0 / 255.0 one)."""
    src, dst = (2160, 3840), (1080, 1920)
    frames, exp = _case(src, dst)
    got, how = _resize(frames, dst)
    assert how == {"resize16": "k_resize16_fused<rows=8,cols=64>", "lds": "23040", "frames": "2"}, how
    assert int((_bits(got) != _bits(exp)).sum()) == 0, int((_bits(got) != _bits(exp)).sum())


def test_bad_arguments_return_the_stated_codes():
    """uint8 frames are UNSUPPORTED (create and run); a wrong shape, dtype of `out` or device is a ValueError; sizes < 1, bad options,
    n = 0, a null frame and short strides are INVALID; each leaves a message."""
    import torch
    from pythoncrt_amd import ResizeHalf
    from pythoncrt_amd._lib import CrtfxError
    with pytest.raises(CrtfxError) as e:
        ResizeHalf(_dev(), (8, 8), (16, 16), pix_fmt=_lib.PIX_U8)
    assert e.value.code == _lib.E_UNSUPPORTED and "half" in str(e.value)
    with pytest.raises(CrtfxError) as e:
        ResizeHalf(_dev(), (8, 8), (0, 16))
    assert e.value.code == _lib.E_INVALID
    with pytest.raises(ValueError):
        ResizeHalf("cpu", (8, 8), (16, 16))
    plan = ResizeHalf(_dev(), (8, 8), (16, 16))
    with pytest.raises(CrtfxError) as e:
        plan.run(torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=_dev()))
    assert e.value.code == _lib.E_UNSUPPORTED and "IngestResize" in str(e.value)
    with pytest.raises(CrtfxError):
        plan.run(torch.zeros((1, 8, 8, 3), dtype=torch.float32, device=_dev()))
    with pytest.raises(ValueError):
        plan.run(torch.zeros((1, 8, 9, 3), dtype=torch.float16, device=_dev()))
    with pytest.raises(ValueError):
        plan.run(torch.zeros((1, 8, 8, 3), dtype=torch.float16))                                   # a host tensor
    with pytest.raises(ValueError):
        plan.run(torch.zeros((1, 8, 8, 3), dtype=torch.float16, device=_dev()), out=torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device=_dev()))
    with pytest.raises(ValueError):
        plan.run(torch.zeros((1, 8, 3, 8), dtype=torch.float16, device=_dev()).transpose(2, 3))     # frames that are not contiguous
    assert tuple(plan.run(torch.zeros((0, 8, 8, 3), dtype=torch.float16, device=_dev())).shape) == (0, 16, 16, 3)
    with pytest.raises(CrtfxError) as e:
        plan.set_option(99, 1)
    assert e.value.code == _lib.E_INVALID and "option" in str(e.value)
    with pytest.raises(CrtfxError) as e:
        plan.set_option(_lib.RESIZE16_OPT_FORCE_GENERAL, 2)
    assert e.value.code == _lib.E_INVALID
    lib = plan.lib
    src = torch.zeros((1, 8, 8, 3), dtype=torch.float16, device=_dev())
    out = torch.zeros((1, 16, 16, 3), dtype=torch.float16, device=_dev())
    st = torch.cuda.current_stream().cuda_stream
    assert lib.crtfx_resize16_run(plan._plan, src.data_ptr(), 384, out.data_ptr(), 1536, 0, st) == _lib.E_INVALID
    assert b"n = 0" in lib.crtfx_resize16_last_error(plan._plan)
    assert lib.crtfx_resize16_run(plan._plan, None, 384, out.data_ptr(), 1536, 1, st) == _lib.E_INVALID
    assert lib.crtfx_resize16_run(plan._plan, src.data_ptr(), 200, out.data_ptr(), 1536, 2, st) == _lib.E_INVALID
    assert b"strides" in lib.crtfx_resize16_last_error(plan._plan)
    if torch.cuda.device_count() > 1:
        with torch.cuda.device(1):
            assert lib.crtfx_resize16_run(plan._plan, src.data_ptr(), 384, out.data_ptr(), 1536, 1, None) == _lib.E_INVALID
            assert b"current device" in lib.crtfx_resize16_last_error(plan._plan)
    buf = ctypes.create_string_buffer(10)
    assert lib.crtfx_resize16_last_plan(plan._plan, buf, 10) == _lib.OK and buf.value == b"resize16="    # truncated, NUL-terminated
    plan.close()
    plan.close()
