"""The source stage on the GPU: UnpackYuv (k_unpack_420, vec and general path, yuv420p and nv12) against the integer host model of
tests/unpack_model.py — equality means zero differing bytes — and process_frames / the CLI with a 4:2:0 input against their own rgb24 path
fed the model's RGB of the same frames."""
import numpy as np
import pytest

from pythoncrt_amd import _lib
from tests import unpack_model as model
from tests import yuv_model

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (2, 2), (3, 5), (16, 64), (34, 132), (37, 131), (270, 480)]
LAYOUTS = ["yuv420p", "nv12"]


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _name(layout, vec):
    return f"k_unpack_420<{layout},{'vec' if vec else 'general'}>"


def _frames(size, layout, seed=0):
    """The three test frames of a size in `layout`: uint8 [3, frame_bytes]."""
    return np.stack([model.relayout(p, size[0], size[1], layout) for p in model.images(*size, seed=seed)])


def _convert(packed_np, size, layout, force_general=False, matrix="bt601", rng="tv"):
    """(uint8[n, h, w, 3] from the device, the plan) for a stack of packed frames."""
    import torch
    from pythoncrt_amd import UnpackYuv
    plan = UnpackYuv(_dev(), size, layout=layout, matrix=matrix, range=rng)
    if force_general:
        plan.set_option(_lib.UNPACK_OPT_FORCE_GENERAL, 1)
    out = plan.run(torch.from_numpy(packed_np).to(_dev()))
    torch.cuda.synchronize()
    got, how = out.cpu().numpy(), plan.plan()
    assert got.shape == (packed_np.shape[0],) + tuple(size) + (3,)
    plan.close()
    return got, how


def _expect(packed_np, size, layout, matrix="bt601", rng="tv"):
    return np.stack([model.unpack(p, size[0], size[1], layout, matrix, rng) for p in packed_np])


@pytest.mark.parametrize("force_general", [False, True], ids=["default", "general"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_frames_equal_the_model(size, layout, force_general):
    """One pixel, one block, odd sizes, widths that are and are not a multiple of 8, more than one thread block: a random frame, a binary
    0 / 255 one and one of clamp colours and greys as one batch of three, both layouts, the default path and the forced general one.  The
    plan names `vec` exactly where the header's rule allows it (w % 8 == 0; the bases and strides of these tensors are multiples of 4)."""
    packed = _frames(size, layout)
    got, how = _convert(packed, size, layout, force_general)
    exp = _expect(packed, size, layout)
    assert int((got != exp).sum()) == 0, (size, layout, how, int((got != exp).sum()))
    assert how == {"unpack": _name(layout, size[1] % 8 == 0 and not force_general), "frames": "3"}, how


@pytest.mark.parametrize("matrix,rng", model.CASES)
@pytest.mark.parametrize("size", [(37, 131), (16, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_matrix_and_range(size, matrix, rng):
    for layout in LAYOUTS:
        packed = _frames(size, layout, seed=7)
        got, how = _convert(packed, size, layout, matrix=matrix, rng=rng)
        exp = _expect(packed, size, layout, matrix, rng)
        assert int((got != exp).sum()) == 0, (size, layout, matrix, rng, how, int((got != exp).sum()))
    assert exp.min() == 0 and exp.max() == 255


def test_strided_batches_leave_the_padding_alone():
    """n = 5 frames (19 x 40: an odd height under the vec path) that are slices of bigger tensors on both sides.  Odd byte bases, or a stride
    that is no multiple of 4, force `general`; bases and strides that are multiples of 4 allow `vec`.  Every frame right, every byte
    outside the frames untouched."""
    import torch
    from pythoncrt_amd import UnpackYuv
    size, n = (19, 40), 5
    sbytes, dbytes = model.sizes(*size)[2], size[0] * size[1] * 3
    packed = np.random.default_rng(3).integers(0, 256, (n, sbytes), dtype=np.uint8)
    for layout in LAYOUTS:
        exp = _expect(packed, size, layout)
        for s_off, d_off, s_pad, d_pad, vec in ((1, 3, 7, 5, False), (4, 8, 12, 4, True), (0, 0, 0, 0, True), (0, 0, 2, 0, False), (0, 2, 0, 4, False)):
            sbuf = torch.full((s_off + n * (sbytes + s_pad) + 16,), 0xEE, dtype=torch.uint8, device=_dev())
            dbuf = torch.full((d_off + n * (dbytes + d_pad) + 16,), 0x5A, dtype=torch.uint8, device=_dev())
            assert sbuf.data_ptr() % 4 == 0 and dbuf.data_ptr() % 4 == 0
            sview = sbuf[s_off:s_off + n * (sbytes + s_pad)].view(n, sbytes + s_pad)[:, :sbytes]
            dview = dbuf[d_off:d_off + n * (dbytes + d_pad)].view(n, dbytes + d_pad)[:, :dbytes].unflatten(1, size + (3,))
            sview.copy_(torch.from_numpy(packed).to(_dev()))
            plan = UnpackYuv(_dev(), size, layout=layout)
            assert plan.run(sview, out=dview) is dview
            torch.cuda.synchronize()
            assert plan.plan() == {"unpack": _name(layout, vec), "frames": "5"}, (plan.plan(), s_off, d_off, s_pad, d_pad)
            assert np.array_equal(dview.cpu().numpy(), exp), (layout, s_off, d_off)
            keep = torch.ones_like(dbuf, dtype=torch.bool)
            keep[d_off:d_off + n * (dbytes + d_pad)].view(n, dbytes + d_pad)[:, :dbytes] = False
            assert bool((dbuf[keep] == 0x5A).all()), (layout, s_off, d_off)
            y, *_ = plan.planes(sview)
            assert tuple(y.shape) == (n,) + size
            plan.close()


def test_one_full_size_batch():
    h, w = 2160, 3840
    packed = np.random.default_rng(11).integers(0, 256, (2, h * w * 3 // 2), dtype=np.uint8)
    got, how = _convert(packed, (h, w), "yuv420p")
    assert how == {"unpack": _name("yuv420p", True), "frames": "2"} and got.shape == (2, h, w, 3)
    exp = _expect(packed, (h, w), "yuv420p")
    assert int((got != exp).sum()) == 0, int((got != exp).sum())


def test_bad_arguments_return_the_stated_codes():
    import torch
    from pythoncrt_amd import UnpackYuv
    from pythoncrt_amd._lib import CrtfxError
    with pytest.raises(CrtfxError) as e:
        UnpackYuv(_dev(), (8, 8), pix_fmt=_lib.PIX_F16)
    assert e.value.code == _lib.E_UNSUPPORTED and "uint8" in str(e.value)
    with pytest.raises(CrtfxError) as e:
        UnpackYuv(_dev(), (0, 16))
    assert e.value.code == _lib.E_INVALID
    with pytest.raises(ValueError):
        UnpackYuv(_dev(), (8, 8), layout="yuv444p")
    plan = UnpackYuv(_dev(), (8, 8))
    assert plan.frame_bytes == 96 and plan.plan() == {"unpack": _name("yuv420p", True), "frames": "0"}
    with pytest.raises(CrtfxError) as e:
        plan.run(torch.zeros((1, 96), dtype=torch.float16, device=_dev()))                  # half input
    assert e.value.code == _lib.E_UNSUPPORTED
    with pytest.raises(ValueError):
        plan.run(torch.zeros((1, 97), dtype=torch.uint8, device=_dev()))                    # a wrong shape
    with pytest.raises(ValueError):
        plan.run(torch.zeros((1, 96), dtype=torch.uint8, device=_dev()), out=torch.zeros((1, 8, 9, 3), dtype=torch.uint8, device=_dev()))
    assert tuple(plan.run(torch.zeros((0, 96), dtype=torch.uint8, device=_dev())).shape) == (0, 8, 8, 3)
    with pytest.raises(CrtfxError) as e:
        plan.set_option(99, 1)
    assert e.value.code == _lib.E_INVALID and "option" in str(e.value)
    lib = plan.lib
    src = torch.zeros((2, 96), dtype=torch.uint8, device=_dev())
    out = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=_dev())
    st = torch.cuda.current_stream().cuda_stream
    assert lib.crtfx_unpack_run(plan._plan, src.data_ptr(), 96, out.data_ptr(), 192, 0, st) == _lib.E_INVALID
    assert b"n = 0" in lib.crtfx_unpack_last_error(plan._plan)
    assert lib.crtfx_unpack_run(plan._plan, None, 96, out.data_ptr(), 192, 1, st) == _lib.E_INVALID
    assert lib.crtfx_unpack_run(plan._plan, src.data_ptr(), 96, None, 192, 1, st) == _lib.E_INVALID
    assert lib.crtfx_unpack_run(plan._plan, src.data_ptr(), 95, out.data_ptr(), 192, 2, st) == _lib.E_INVALID
    assert b"strides" in lib.crtfx_unpack_last_error(plan._plan)
    assert lib.crtfx_unpack_run(plan._plan, src.data_ptr(), 96, out.data_ptr(), 191, 2, st) == _lib.E_INVALID
    torch.cuda.synchronize()
    assert int(out.sum()) == 0                                                              # no refused call wrote anything
    plan.close()


# ---- process_frames ------------------------------------------------------------------------------------------------------------------------------

def _render(frames, out_hw=(36, 64), batch=4, **kw):
    import pythoncrt_amd as pc
    got = []
    n = pc.process_frames(iter(frames), lambda a: got.append(np.array(a)), out_hw[1], out_hw[0], 30.0, len(frames), noise_seed=5, batch=batch, **kw)
    return n, got


def _same(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and np.array_equal(x, y), (i, int((x != y).sum()))


def test_process_frames_takes_yuv_frames_as_it_takes_their_rgb():
    """Six 36 x 64 frames in batches of four (a full batch and a short one; persistence on, the grain fixed by noise_seed): the frames written
    for a 4:2:0 input equal those of the rgb24 path fed the model's RGB of the same frames — nv12 with the defaults, yuv420p with bt709 /
    pc, and with out_pix_fmt="nv12" on top both ends are 4:2:0.  Items of any shape are flattened."""
    rng = np.random.default_rng(41)
    fb = model.sizes(36, 64)[2]
    packed = [rng.integers(0, 256, fb, dtype=np.uint8) for _ in range(6)]
    for fmt, kw, mkw in (("nv12", {}, {}), ("yuv420p", dict(in_matrix="bt709", in_range="pc"), dict(matrix="bt709", rng="pc"))):
        rgb = [model.unpack(p, 36, 64, fmt, **mkw) for p in packed]
        n_rgb, want = _render(rgb)
        n_yuv, got = _render([p.reshape(3, -1) for p in packed], in_pix_fmt=fmt, **kw)
        assert n_rgb == n_yuv == 6 and want[0].shape == (36, 64, 3)
        _same(got, want)
        assert not np.array_equal(got[0], got[1])
        if fmt == "nv12":
            n_both, both = _render(packed, in_pix_fmt="nv12", out_pix_fmt="nv12")
            assert n_both == 6
            _same(both, [yuv_model.pack(a, "nv12") for a in want])


def test_process_frames_resizes_an_off_size_yuv_source_on_the_device():
    """in_size = (18, 32) against a 36 x 64 output: the frames equal the rgb24 call fed the model's 18 x 32 RGB with resize_on="device"."""
    rng = np.random.default_rng(42)
    fb = model.sizes(18, 32)[2]
    packed = [rng.integers(0, 256, fb, dtype=np.uint8) for _ in range(6)]
    _, want = _render([model.unpack(p, 18, 32, "nv12") for p in packed], resize_on="device")
    n, got = _render(packed, in_pix_fmt="nv12", in_size=(18, 32))
    assert n == 6
    _same(got, want)


def test_process_frames_refuses_what_it_cannot_take():
    fb = model.sizes(36, 64)[2]
    good = [np.zeros(fb, dtype=np.uint8)]
    with pytest.raises(ValueError, match="in_pix_fmt"):
        _render(good, in_pix_fmt="yuv444p")
    with pytest.raises(ValueError, match="host"):
        _render(good, in_pix_fmt="nv12", resize_on="host")
    with pytest.raises(ValueError) as e:
        _render([np.zeros(fb - 1, dtype=np.uint8)], in_pix_fmt="nv12")
    assert str(fb) in str(e.value) and str(fb - 1) in str(e.value)
    with pytest.raises(ValueError) as e:
        _render([np.zeros((36, 64, 3), dtype=np.uint8)], in_pix_fmt="yuv420p")           # an rgb24 frame where a 4:2:0 one is due
    assert str(fb) in str(e.value) and str(36 * 64 * 3) in str(e.value)


# ---- CLI ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("io", ["staged", "mapped"])
def test_cli_yuv420p_input_is_the_rgb24_run_on_the_models_rgb(tmp_path, io):
    """--in-pix-fmt yuv420p over a 3-frame 38 x 72 file (batch 2: a full batch and a short one), --io staged and --io mapped: the output
    equals the rgb24-input run on the model's RGB of that file, byte for byte; with --in-pix-fmt nv12 --out-pix-fmt nv12 together the
    output is yuv_model.pack of the rgb run's frames."""
    from pythoncrt_amd import cli
    n, h, w = 3, 38, 72
    fb = model.sizes(h, w)[2]
    packed = np.random.default_rng(43).integers(0, 256, (n, fb), dtype=np.uint8)
    rgb = np.stack([model.unpack(p, h, w, "yuv420p") for p in packed])
    (tmp_path / "in.yuv").write_bytes(packed.tobytes())
    (tmp_path / "in.nv12").write_bytes(np.stack([model.relayout(p, h, w, "nv12") for p in packed]).tobytes())
    (tmp_path / "in.rgb").write_bytes(rgb.tobytes())
    flags = ["--width", str(w), "--height", str(h), "--fps", "30", "--batch", "2", "--noise-seed", "17", "--persistence", "0.3", "--io", io]
    assert cli.main(flags + ["--input", str(tmp_path / "in.rgb"), "--output", str(tmp_path / "out_rgb.rgb")]) == 0
    assert cli.main(flags + ["--input", str(tmp_path / "in.yuv"), "--output", str(tmp_path / "out_yuv.rgb"), "--in-pix-fmt", "yuv420p", "--staging-report"]) == 0
    want = (tmp_path / "out_rgb.rgb").read_bytes()
    got = (tmp_path / "out_yuv.rgb").read_bytes()
    assert len(want) == len(got) == n * h * w * 3
    assert got == want, int((np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8)).sum())
    assert cli.main(flags + ["--input", str(tmp_path / "in.nv12"), "--output", str(tmp_path / "out.nv12"), "--in-pix-fmt", "nv12", "--out-pix-fmt", "nv12"]) == 0
    both = np.frombuffer((tmp_path / "out.nv12").read_bytes(), dtype=np.uint8)
    frames = np.frombuffer(want, dtype=np.uint8).reshape(n, h, w, 3)
    assert both.size == n * fb
    for i in range(n):
        exp = yuv_model.pack(frames[i], "nv12")
        assert np.array_equal(both.reshape(n, fb)[i], exp), (io, i, int((both.reshape(n, fb)[i] != exp).sum()))
