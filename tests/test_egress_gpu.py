"""The egress stage on the GPU: EgressYuv (k_egress_420, vec and general path, yuv420p and nv12) against the integer host model of
tests/yuv_model.py — equality means zero differing bytes — and process_frames / the CLI with a 4:2:0 output against the model applied to
their own rgb24 output."""
import numpy as np
import pytest

from pythoncrt_amd import _lib
from tests import yuv_model as model

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (2, 2), (3, 5), (16, 64), (34, 132), (37, 131), (270, 480)]
LAYOUTS = ["yuv420p", "nv12"]


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _name(layout, vec):
    return f"k_egress_420<{layout},{'vec' if vec else 'general'}>"


def _convert(frames_np, layout, force_general=False, matrix="bt601", rng="tv"):
    """(uint8[n, frame_bytes] from the device, the plan) for a stack of equal-size frames."""
    import torch
    from pythoncrt_amd import EgressYuv
    plan = EgressYuv(_dev(), frames_np.shape[1:3], layout=layout, matrix=matrix, range=rng)
    if force_general:
        plan.set_option(_lib.EGRESS_OPT_FORCE_GENERAL, 1)
    out = plan.run(torch.from_numpy(frames_np).to(_dev()))
    torch.cuda.synchronize()
    got, how = out.cpu().numpy(), plan.plan()
    assert got.shape == (frames_np.shape[0], plan.frame_bytes)
    plan.close()
    return got, how


def _expect(frames_np, layout, matrix="bt601", rng="tv"):
    return np.stack([model.pack(f, layout, matrix, rng) for f in frames_np])


@pytest.mark.parametrize("force_general", [False, True], ids=["default", "general"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_frames_equal_the_model(size, layout, force_general):
    """One pixel, one block, odd sizes, widths that are and are not a multiple of 8, more than one thread block: a random frame, a binary
    0 / 255 one and one of clamp colours and greys as one batch of three, both layouts, the default path and the forced general one.  The
    plan names `vec` exactly where the header's rule allows it (w % 8 == 0; the bases and strides of these tensors are multiples of 4)."""
    frames = model.images(*size)
    got, how = _convert(frames, layout, force_general)
    exp = _expect(frames, layout)
    assert int((got != exp).sum()) == 0, (size, layout, how, int((got != exp).sum()))
    assert how == {"egress": _name(layout, size[1] % 8 == 0 and not force_general), "frames": "3"}, how


@pytest.mark.parametrize("matrix,rng", model.CASES)
@pytest.mark.parametrize("size", [(37, 131), (16, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_matrix_and_range(size, matrix, rng):
    frames = model.images(*size, seed=7)
    for layout in LAYOUTS:
        got, how = _convert(frames, layout, matrix=matrix, rng=rng)
        exp = _expect(frames, layout, matrix, rng)
        assert int((got != exp).sum()) == 0, (size, layout, matrix, rng, how, int((got != exp).sum()))
    if rng == "pc":                                                          # the clamp colours are in the third frame: 255, not 256 & 255 = 0
        assert exp[2].max() == 255


def test_strided_batches_leave_the_padding_alone():
    """n = 5 frames (19 x 40: an odd height under the vec path) that are slices of bigger tensors on both sides.  Odd byte bases, or a stride
    that is no multiple of 4, force `general`; bases and strides that are multiples of 4 allow `vec`.  Every frame right, every byte
    outside the frames untouched."""
    import torch
    from pythoncrt_amd import EgressYuv
    size, n = (19, 40), 5
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (n,) + size + (3,), dtype=np.uint8)
    sbytes, dbytes = size[0] * size[1] * 3, model.sizes(*size)[2]
    for layout in LAYOUTS:
        exp = _expect(frames, layout)
        for s_off, d_off, s_pad, d_pad, vec in ((1, 3, 7, 5, False), (4, 8, 12, 4, True), (0, 0, 0, 0, True), (0, 0, 2, 0, False), (0, 2, 0, 4, False)):
            sbuf = torch.full((s_off + n * (sbytes + s_pad) + 16,), 0xEE, dtype=torch.uint8, device=_dev())
            dbuf = torch.full((d_off + n * (dbytes + d_pad) + 16,), 0x5A, dtype=torch.uint8, device=_dev())
            assert sbuf.data_ptr() % 4 == 0 and dbuf.data_ptr() % 4 == 0
            sview = sbuf[s_off:s_off + n * (sbytes + s_pad)].view(n, sbytes + s_pad)[:, :sbytes].unflatten(1, size + (3,))
            dview = dbuf[d_off:d_off + n * (dbytes + d_pad)].view(n, dbytes + d_pad)[:, :dbytes]
            sview.copy_(torch.from_numpy(frames).to(_dev()))
            plan = EgressYuv(_dev(), size, layout=layout)
            assert plan.run(sview, out=dview) is dview
            torch.cuda.synchronize()
            assert plan.plan() == {"egress": _name(layout, vec), "frames": "5"}, (plan.plan(), s_off, d_off, s_pad, d_pad)
            assert np.array_equal(dview.cpu().numpy(), exp), (layout, s_off, d_off)
            keep = torch.ones_like(dbuf, dtype=torch.bool)
            keep[d_off:d_off + n * (dbytes + d_pad)].view(n, dbytes + d_pad)[:, :dbytes] = False
            assert bool((dbuf[keep] == 0x5A).all()), (layout, s_off, d_off)
            y, *_ = plan.planes(dview)
            assert tuple(y.shape) == (n,) + size
            plan.close()


def test_one_full_size_batch():
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (2, 2160, 3840, 3), dtype=np.uint8)
    got, how = _convert(frames, "yuv420p")
    assert how == {"egress": _name("yuv420p", True), "frames": "2"} and got.shape == (2, 2160 * 3840 * 3 // 2)
    exp = _expect(frames, "yuv420p")
    assert int((got != exp).sum()) == 0, int((got != exp).sum())


def test_bad_arguments_return_the_stated_codes():
    import torch
    from pythoncrt_amd import EgressYuv
    from pythoncrt_amd._lib import CrtfxError
    with pytest.raises(CrtfxError) as e:
        EgressYuv(_dev(), (8, 8), pix_fmt=_lib.PIX_F16)
    assert e.value.code == _lib.E_UNSUPPORTED and "uint8" in str(e.value)
    with pytest.raises(CrtfxError) as e:
        EgressYuv(_dev(), (0, 16))
    assert e.value.code == _lib.E_INVALID
    with pytest.raises(ValueError):
        EgressYuv(_dev(), (8, 8), layout="yuv444p")
    plan = EgressYuv(_dev(), (8, 8))
    assert plan.frame_bytes == 96 and plan.plan() == {"egress": _name("yuv420p", True), "frames": "0"}
    with pytest.raises(CrtfxError) as e:
        plan.run(torch.zeros((1, 8, 8, 3), dtype=torch.float16, device=_dev()))
    assert e.value.code == _lib.E_UNSUPPORTED
    with pytest.raises(ValueError):
        plan.run(torch.zeros((1, 8, 9, 3), dtype=torch.uint8, device=_dev()))
    with pytest.raises(CrtfxError) as e:
        plan.set_option(99, 1)
    assert e.value.code == _lib.E_INVALID and "option" in str(e.value)
    lib = plan.lib
    src = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=_dev())
    out = torch.zeros((2, 96), dtype=torch.uint8, device=_dev())
    st = torch.cuda.current_stream().cuda_stream
    assert lib.crtfx_egress_run(plan._plan, src.data_ptr(), 192, out.data_ptr(), 96, 0, st) == _lib.E_INVALID
    assert b"n = 0" in lib.crtfx_egress_last_error(plan._plan)
    assert lib.crtfx_egress_run(plan._plan, None, 192, out.data_ptr(), 96, 1, st) == _lib.E_INVALID
    assert lib.crtfx_egress_run(plan._plan, src.data_ptr(), 192, out.data_ptr(), 95, 2, st) == _lib.E_INVALID
    assert b"strides" in lib.crtfx_egress_last_error(plan._plan)
    plan.close()


# ---- process_frames ------------------------------------------------------------------------------------------------------------------------------

def _render(frames, out_pix_fmt, out_hw=(36, 64), batch=4, **kw):
    import pythoncrt_amd as pc
    got = []
    n = pc.process_frames(iter(frames), lambda a: got.append(np.array(a)), out_hw[1], out_hw[0], 30.0, len(frames), noise_seed=5, batch=batch,
                          out_pix_fmt=out_pix_fmt, **kw)
    return n, got


def test_process_frames_nv12_is_the_model_of_its_rgb24_frames():
    """Six 36 x 64 frames in batches of four (a full batch and a short one; persistence on): the nv12 frames the writer receives are the
    model applied to the rgb24 frames of the same call (the grain is counter-based: noise_seed fixes it); every array handed to
    `write_frame` is 1-D with frame_bytes elements."""
    rng = np.random.default_rng(31)
    frames = [rng.integers(0, 256, (36, 64, 3), dtype=np.uint8) for _ in range(6)]
    n_rgb, rgb = _render(frames, "rgb24")
    fb = model.sizes(36, 64)[2]
    for fmt, kw in (("nv12", {}), ("yuv420p", dict(out_matrix="bt709", out_range="pc"))):
        n_yuv, yuv = _render(frames, fmt, **kw)
        assert n_rgb == n_yuv == 6 and len(rgb) == len(yuv) == 6
        for i, (a, b) in enumerate(zip(rgb, yuv)):
            assert a.shape == (36, 64, 3) and b.shape == (fb,) and b.dtype == np.uint8
            exp = model.pack(a, fmt, kw.get("out_matrix", "bt601"), kw.get("out_range", "tv"))
            assert np.array_equal(b, exp), (fmt, i, int((b != exp).sum()))
    assert not np.array_equal(rgb[0], rgb[1])
    with pytest.raises(ValueError, match="out_pix_fmt"):
        _render(frames, "yuv444p")


def test_process_frames_yuv_output_behind_the_ingest_path():
    """The source size changes mid-stream (off-size frames are resized on the device, a batch ends where the size changes): order and bytes
    of the yuv420p output still follow the rgb24 output."""
    rng = np.random.default_rng(32)
    shapes = [(36, 64), (18, 32), (18, 32), (36, 64), (27, 48), (27, 48), (36, 64)]
    frames = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in shapes]
    kw = dict(persistence=0.4, pixel_size=1)
    n_rgb, rgb = _render(frames, "rgb24", **kw)
    n_yuv, yuv = _render(frames, "yuv420p", **kw)
    assert n_rgb == n_yuv == 7
    for i, (a, b) in enumerate(zip(rgb, yuv)):
        assert np.array_equal(b, model.pack(a, "yuv420p")), (i, shapes[i])


# ---- CLI ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("io", ["staged", "mapped"])
def test_cli_yuv420p_file_is_the_model_of_the_rgb24_run(tmp_path, io):
    """--out-pix-fmt yuv420p over a 3-frame file (batch 2: a full batch and a short one), --io staged and --io mapped: the file holds
    3 * frame_bytes bytes, each frame the model of the rgb24 run's frame."""
    from pythoncrt_amd import cli
    n, h, w = 3, 38, 72
    rng = np.random.default_rng(33)
    frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    src = tmp_path / "in.rgb"
    src.write_bytes(frames.tobytes())
    flags = ["--input", str(src), "--width", str(w), "--height", str(h), "--fps", "30", "--batch", "2", "--noise-seed", "17", "--persistence", "0.3",
             "--io", io]
    assert cli.main(flags + ["--output", str(tmp_path / "out.rgb")]) == 0
    assert cli.main(flags + ["--output", str(tmp_path / "out.yuv"), "--out-pix-fmt", "yuv420p", "--staging-report"]) == 0
    rgb = np.frombuffer((tmp_path / "out.rgb").read_bytes(), dtype=np.uint8).reshape(n, h, w, 3)
    fb = model.sizes(h, w)[2]
    raw = (tmp_path / "out.yuv").read_bytes()
    assert len(raw) == n * fb
    yuv = np.frombuffer(raw, dtype=np.uint8).reshape(n, fb)
    for i in range(n):
        exp = model.pack(rgb[i], "yuv420p")
        assert np.array_equal(yuv[i], exp), (io, i, int((yuv[i] != exp).sum()))
