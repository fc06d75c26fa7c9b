"""The ingest stage on the GPU: IngestResize (k_ingest_fused, and k_ingest_h + k_ingest_v) against the installed Pillow's
`Image.resize((w, h), Image.BILINEAR)` — equality everywhere — and process_frames(resize_on="device") against resize_on="host"."""
import ctypes

import numpy as np
import pytest

from pythoncrt_amd import _lib
from tests import pil_resize_model as model

pytestmark = pytest.mark.gpu

FUSED, GENERAL = "k_ingest_fused<", "k_ingest_h+k_ingest_v"


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _resize(src_np, dst, force_general=False):
    """(uint8[n, h, w, 3] from the device, the plan string) for a stack of equal-size frames."""
    import torch
    from pythoncrt_amd import IngestResize
    plan = IngestResize(_dev(), src_np.shape[1:3], dst)
    if force_general:
        plan.set_option(_lib.INGEST_OPT_FORCE_GENERAL, 1)
    out = plan.run(torch.from_numpy(src_np).to(_dev()))
    torch.cuda.synchronize()
    got, how = out.cpu().numpy(), plan.plan()
    plan.close()
    return got, how


def _expect(src_np, dst):
    return np.stack([model.pillow(f, *dst) for f in src_np])


@pytest.mark.parametrize("force_general", [False, True], ids=["default", "general"])
@pytest.mark.parametrize("src,dst", model.PAIRS + model.EXTRA_PAIRS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_resize_equals_pillow(src, dst, force_general):
    """Every pair of the CPU list plus the 1/40 reduction and the four ragged widths (row starts on every byte offset mod 4, heights that
    are no multiple of a tile), both images as one batch of two, both paths; the plan names the path that ran."""
    imgs = model.images(*src)
    frames = np.stack([imgs["random"], imgs["binary"]])
    got, how = _resize(frames, dst, force_general)
    exp = _expect(frames, dst)
    assert got.shape == exp.shape
    assert int((got != exp).sum()) == 0, (src, dst, how, int((got != exp).sum()))
    assert how["frames"] == "2"
    if force_general:
        assert how["ingest"] == GENERAL, how
    elif (src, dst) == ((360, 640), (9, 16)):
        assert how["ingest"] == GENERAL, how                   # 81 taps per axis: no tile fits the LDS budget
    else:
        assert how["ingest"].startswith(FUSED) and 0 < int(how["lds"]) <= 40960, how


def test_both_paths_are_taken_by_default_somewhere():
    from pythoncrt_amd import IngestResize
    a, b = IngestResize(_dev(), (360, 640), (9, 16)), IngestResize(_dev(), (1080, 1920), (2160, 3840))
    assert a.plan()["ingest"] == GENERAL and b.plan()["ingest"] == "k_ingest_fused<rows=32,cols=128>", (a.plan(), b.plan())
    c = IngestResize(_dev(), (2160, 3840), (540, 960))          # the header's rule: every ratio down to 1/4 is fused
    assert c.plan()["ingest"].startswith(FUSED), c.plan()


def test_strided_batches_leave_the_padding_alone():
    """n = 5 frames that are slices of bigger tensors on both sides (strides larger than a frame, starting at odd byte addresses): every
    frame right, every byte outside the frames untouched — on both paths."""
    import torch
    src, dst, n = (45, 80), (67, 123), 5
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (n,) + src + (3,), dtype=np.uint8)
    exp = _expect(frames, dst)
    sbytes, dbytes = src[0] * src[1] * 3, dst[0] * dst[1] * 3
    from pythoncrt_amd import IngestResize
    for force in (0, 1):
        for s_off, d_off, s_pad, d_pad in ((1, 3, 7, 5), (2, 1, 64, 1), (0, 0, 0, 0)):
            sbuf = torch.full((s_off + n * (sbytes + s_pad) + 16,), 0xEE, dtype=torch.uint8, device=_dev())
            dbuf = torch.full((d_off + n * (dbytes + d_pad) + 16,), 0x5A, dtype=torch.uint8, device=_dev())
            sview = sbuf[s_off:s_off + n * (sbytes + s_pad)].view(n, sbytes + s_pad)[:, :sbytes].unflatten(1, src + (3,))
            dview = dbuf[d_off:d_off + n * (dbytes + d_pad)].view(n, dbytes + d_pad)[:, :dbytes].unflatten(1, dst + (3,))
            sview.copy_(torch.from_numpy(frames).to(_dev()))
            plan = IngestResize(_dev(), src, dst)
            plan.set_option(_lib.INGEST_OPT_FORCE_GENERAL, force)
            assert plan.run(sview, out=dview) is dview
            torch.cuda.synchronize()
            assert plan.plan()["frames"] == "5" and (plan.plan()["ingest"] == GENERAL) == bool(force)
            assert np.array_equal(dview.cpu().numpy(), exp), (force, s_off, d_off)
            keep = torch.ones_like(dbuf, dtype=torch.bool)
            keep[d_off:d_off + n * (dbytes + d_pad)].view(n, dbytes + d_pad)[:, :dbytes] = False
            assert bool((dbuf[keep] == 0x5A).all()), (force, s_off, d_off)
            plan.close()


@pytest.mark.parametrize("src,dst", [((1080, 1920), (2160, 3840)), ((720, 1280), (1080, 1920)), ((2160, 3840), (1080, 1920))],
                         ids=["1080p-4K", "720p-1080p", "4K-1080p"])
def test_full_size_frames(src, dst):
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (1,) + src + (3,), dtype=np.uint8)
    exp = _expect(frames, dst)
    for force in (False, True):
        got, how = _resize(frames, dst, force)
        assert int((got != exp).sum()) == 0, (src, dst, how, int((got != exp).sum()))
        assert (how["ingest"] == GENERAL) == force, how


def test_bad_arguments_return_the_stated_codes():
    """fp16 frames are UNSUPPORTED (create and run); sizes < 1, a device that is not current and bad options are INVALID; each leaves a message."""
    import torch
    from pythoncrt_amd import IngestResize
    from pythoncrt_amd._lib import CrtfxError
    with pytest.raises(CrtfxError) as e:
        IngestResize(_dev(), (8, 8), (16, 16), pix_fmt=_lib.PIX_F16)
    assert e.value.code == _lib.E_UNSUPPORTED and "uint8" in str(e.value)
    with pytest.raises(CrtfxError) as e:
        IngestResize(_dev(), (8, 8), (0, 16))
    assert e.value.code == _lib.E_INVALID
    plan = IngestResize(_dev(), (8, 8), (16, 16))
    with pytest.raises(CrtfxError) as e:
        plan.run(torch.zeros((1, 8, 8, 3), dtype=torch.float16, device=_dev()))
    assert e.value.code == _lib.E_UNSUPPORTED
    with pytest.raises(ValueError):
        plan.run(torch.zeros((1, 8, 9, 3), dtype=torch.uint8, device=_dev()))
    with pytest.raises(CrtfxError) as e:
        plan.set_option(99, 1)
    assert e.value.code == _lib.E_INVALID and "option" in str(e.value)
    lib = plan.lib
    src = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=_dev())
    out = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device=_dev())
    st = torch.cuda.current_stream().cuda_stream
    assert lib.crtfx_ingest_run(plan._plan, src.data_ptr(), 192, out.data_ptr(), 768, 0, st) == _lib.E_INVALID
    assert b"n = 0" in lib.crtfx_ingest_last_error(plan._plan)
    assert lib.crtfx_ingest_run(plan._plan, None, 192, out.data_ptr(), 768, 1, st) == _lib.E_INVALID
    assert lib.crtfx_ingest_run(plan._plan, src.data_ptr(), 100, out.data_ptr(), 768, 2, st) == _lib.E_INVALID
    assert b"strides" in lib.crtfx_ingest_last_error(plan._plan)
    if torch.cuda.device_count() > 1:
        with torch.cuda.device(1):
            assert lib.crtfx_ingest_run(plan._plan, src.data_ptr(), 192, out.data_ptr(), 768, 1, None) == _lib.E_INVALID
            assert b"current device" in lib.crtfx_ingest_last_error(plan._plan)
    buf = ctypes.create_string_buffer(8)
    assert lib.crtfx_ingest_last_plan(plan._plan, buf, 8) == _lib.OK and buf.value == b"ingest="      # truncated, NUL-terminated
    plan.close()


# ---- process_frames ------------------------------------------------------------------------------------------------------------------------------

def _render(frames, resize_on, out_hw=(135, 240), batch=4, total=True, **kw):
    import pythoncrt_amd as pc
    got, prog = [], []
    n = pc.process_frames(iter(frames), lambda a: got.append(a.copy()), out_hw[1], out_hw[0], 30.0, len(frames) if total else None,
                          noise_seed=5, batch=batch, resize_on=resize_on, progress_cb=prog.append, **kw)
    return n, got, prog


def _config_keywords(n):
    from pythoncrt_amd.pipeline import baseline_config
    rs = baseline_config(n)[0]
    import inspect
    import pythoncrt_amd as pc
    names = set(inspect.signature(pc.process_frames).parameters)
    return {k: v for k, v in vars(rs).items() if k in names}


@pytest.mark.parametrize("settings", ["cli_default", "config2", "config4"])
def test_process_frames_device_resize_equals_host_resize(settings):
    """A 90x160 source into a 135x240 render: the frames the writer receives are the same bytes whether the frames are resized by the
    ingest kernels or by Pillow on the host (the grain is counter-based: noise_seed fixes it).  Settings: the CLI's defaults (fast bloom,
    pixelate, persistence 0.2), BASELINE config 2's (Gaussian bloom, warp) and config 4's (config 2's with persistence 0.5): with a
    persistence chain a wrong frame would corrupt its successors too."""
    import inspect
    import pythoncrt_amd as pc
    kw = {} if settings == "cli_default" else _config_keywords(int(settings[-1]))
    if settings != "config2":
        assert kw.get("persistence", inspect.signature(pc.process_frames).parameters["persistence"].default) > 0
    rng = np.random.default_rng(21)
    frames = [rng.integers(0, 256, (90, 160, 3), dtype=np.uint8) for _ in range(7)]
    nd, dev_frames, dev_prog = _render(frames, "device", **kw)
    nh, host_frames, host_prog = _render(frames, "host", **kw)
    assert nd == nh == 7 and len(dev_frames) == len(host_frames) == 7 and dev_prog == host_prog == [min(1.0, (i + 1) / 7) for i in range(7)]
    for i, (a, b) in enumerate(zip(dev_frames, host_frames)):
        assert a.shape == (135, 240, 3) and np.array_equal(a, b), (settings, i, int((a != b).sum()))
    assert not np.array_equal(dev_frames[0], dev_frames[1])


def test_process_frames_mixed_source_sizes_across_batches():
    """Eleven frames, batch 4, three source sizes and the output size itself, changing inside and at batch boundaries: count, order, bytes
    and progress calls as with the host resize (persistence on, so order matters)."""
    rng = np.random.default_rng(22)
    sizes = [(90, 160), (90, 160), (135, 240), (54, 96), (54, 96), (54, 96), (54, 96), (54, 96), (270, 480), (135, 240), (90, 160)]
    frames = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in sizes]
    kw = dict(persistence=0.4, pixel_size=1)
    nd, dev_frames, dev_prog = _render(frames, "device", **kw)
    nh, host_frames, host_prog = _render(frames, "host", **kw)
    assert nd == nh == 11 and dev_prog == host_prog and len(dev_prog) == 11
    for i, (a, b) in enumerate(zip(dev_frames, host_frames)):
        assert np.array_equal(a, b), (i, sizes[i], int((a != b).sum()))
    # more source sizes than the loop keeps plans for, and no total: one closing progress call
    sizes = [(20 + 3 * i, 40 + 5 * i) for i in range(6)] * 2
    frames = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in sizes]
    nd, dev_frames, dev_prog = _render(frames, "device", total=False, **kw)
    nh, host_frames, _ = _render(frames, "host", total=False, **kw)
    assert nd == nh == 12 and dev_prog == [1.0] and all(np.array_equal(a, b) for a, b in zip(dev_frames, host_frames))


def test_process_frames_writer_failure_drains_and_bad_keyword():
    import torch
    import pythoncrt_amd as pc
    rng = np.random.default_rng(23)
    frames = [rng.integers(0, 256, (90, 160, 3), dtype=np.uint8) for _ in range(11)]
    seen = []

    def writer(a):
        if len(seen) == 5:
            raise OSError("encoder pipe closed")
        seen.append(a.copy())

    with pytest.raises(OSError, match="encoder pipe closed"):
        pc.process_frames(iter(frames), writer, 240, 135, 30.0, 11, noise_seed=5, batch=4)
    torch.cuda.synchronize()
    _, good, _ = _render(frames, "host")
    assert len(seen) == 5 and all(np.array_equal(a, b) for a, b in zip(seen, good))
    with pytest.raises(ValueError, match="resize_on"):
        pc.process_frames(iter(frames), writer, 240, 135, 30.0, 11, resize_on="gpu")
