"""The 8-bit 4:2:2 pair on the GPU: UnpackYuv422 (k_unpack_422) and EgressYuv422 (k_egress_422), vec and general path, yuv422p, yuyv422 and
uyvy422, against the integer host model of tests/yuv422_model.py byte for byte, and process_frames / the CLI with 4:2:2 formats against the
model wrapped round the rgb24 run with the same seed."""
import numpy as np
import pytest

from pythoncrt_amd import _lib
from tests import yuv422_model as model
from tests import yuv_model

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (2, 2), (3, 5), (16, 64), (34, 132), (37, 131), (270, 480)]
VEC_SIZES = {(16, 64), (270, 480)}
LAYOUTS = list(model.LAYOUTS)


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _name(kind, layout, vec):
    return f"{kind}422=k_{kind}_422<{layout},{'vec' if vec else 'general'}>"


def _unpack(packed_np, size, layout, force_general=False, matrix="bt601", rng="tv"):
    """(uint8[n, h, w, 3] from the device, last_plan) for a stack of packed frames."""
    import torch
    from pythoncrt_amd import UnpackYuv422
    plan = UnpackYuv422(_dev(), size, layout, matrix=matrix, rng=rng)
    plan.force_general = force_general
    out = plan(torch.from_numpy(packed_np).to(_dev()))
    torch.cuda.synchronize()
    got, how = out.cpu().numpy(), plan.last_plan()
    assert got.dtype == np.uint8 and got.shape == (packed_np.shape[0],) + tuple(size) + (3,)
    plan.close()
    return got, how


def _egress(frames_np, layout, force_general=False, matrix="bt601", rng="tv"):
    """(uint8[n, frame_bytes] from the device, last_plan) for a stack of RGB frames."""
    import torch
    from pythoncrt_amd import EgressYuv422
    size = tuple(frames_np.shape[1:3])
    plan = EgressYuv422(_dev(), size, layout, matrix=matrix, rng=rng, force_general=force_general)
    out = plan(torch.from_numpy(frames_np).to(_dev()))
    torch.cuda.synchronize()
    got, how = out.cpu().numpy(), plan.last_plan()
    assert got.dtype == np.uint8 and got.shape == (frames_np.shape[0], plan.frame_bytes) and plan.frame_bytes == model.sizes(size[0], size[1], layout)[1]
    plan.close()
    return got, how


def _unpacked(packed_np, size, layout, matrix="bt601", rng="tv"):
    return np.stack([model.unpack(p, size[0], size[1], layout, matrix, rng) for p in packed_np])


def _packed(frames_np, layout, matrix="bt601", rng="tv"):
    return np.stack([model.pack(f, layout, matrix, rng) for f in frames_np])


def _same(got, exp, what):
    bad = int((got != exp).sum())
    assert got.shape == exp.shape and bad == 0, (what, bad)


# ---- both directions: frames equal the model --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("force_general", [False, True], ids=["default", "general"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_source_frames_equal_the_model(size, layout, force_general):
    """One pixel, one pair, odd sizes, widths that are and are not a multiple of 8, more than one thread block: three frames of random
    bytes over all of 0..255, so both clamps are live.  The default run takes vec at 16 x 64 and 270 x 480 and general elsewhere."""
    packed = model.sources(size[0], size[1], layout)
    got, how = _unpack(packed, size, layout, force_general)
    _same(got, _unpacked(packed, size, layout), (size, layout, how))
    assert size[0] * size[1] < 1000 or (got.min() == 0 and got.max() == 255)                 # both clamps acted (not asked of a handful of pixels)
    assert how == _name("unpack", layout, size in VEC_SIZES and not force_general) + ";frames=3", how


@pytest.mark.parametrize("force_general", [False, True], ids=["default", "general"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_egress_frames_equal_the_model(size, layout, force_general):
    """Three frames of random RGB; every output byte is compared, the pad byte of an odd-width packed row included."""
    frames = model.frames(*size)
    got, how = _egress(frames, layout, force_general)
    _same(got, _packed(frames, layout), (size, layout, how))
    assert how == _name("egress", layout, size in VEC_SIZES and not force_general) + ";frames=3", how


@pytest.mark.parametrize("force_general", [False, True], ids=["default", "general"])
@pytest.mark.parametrize("matrix,rng", model.CASES)
@pytest.mark.parametrize("size", [(37, 131), (16, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_matrix_and_range(size, matrix, rng, force_general):
    """Both paths see every matrix at both sizes (the default run is vec at 16 x 64).  At full range the egress frame holds pure blue and pure red pairs: the upper clamp acts (U, V = 256 before it)."""
    frames = model.frames(*size, seed=7)
    frames[:, 0, 0:2] = (0, 0, 255)
    frames[:, 0, 2:4] = (255, 0, 0)
    for layout in LAYOUTS:
        packed = model.sources(size[0], size[1], layout, seed=7)
        vec = "vec" if size in VEC_SIZES and not force_general else "general"
        got, how = _unpack(packed, size, layout, force_general, matrix=matrix, rng=rng)
        _same(got, _unpacked(packed, size, layout, matrix, rng), (size, layout, matrix, rng, how))
        assert f",{vec}>" in how, how
        back, how = _egress(frames, layout, force_general, matrix=matrix, rng=rng)
        _same(back, _packed(frames, layout, matrix, rng), (size, layout, matrix, rng, how))
        assert f",{vec}>" in how, how


def test_one_batch_at_1080p():
    """2 frames of 1080 x 1920: uyvy422 in, yuv422p out, on the vec path."""
    size = (1080, 1920)
    packed = model.sources(size[0], size[1], "uyvy422", n=2)
    got, how = _unpack(packed, size, "uyvy422")
    assert how == _name("unpack", "uyvy422", True) + ";frames=2"
    _same(got, _unpacked(packed, size, "uyvy422"), how)
    back, how = _egress(got, "yuv422p")
    assert how == _name("egress", "yuv422p", True) + ";frames=2"
    _same(back, _packed(got, "yuv422p"), how)


# ---- misaligned bases and strided batches ---------------------------------------------------------------------------------------------------

# (source offset, destination offset, source gap, destination gap, vec?)
STRIDES = [(0, 0, 8, 12, True), (4, 8, 4, 4, True), (1, 0, 4, 4, False), (0, 1, 4, 4, False), (2, 0, 4, 4, False), (0, 2, 4, 4, False),
           (0, 0, 3, 4, False), (0, 0, 4, 5, False), (0, 0, 2, 4, False), (3, 1, 1, 7, False)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", ["unpack", "egress"])
def test_offset_and_strided_batches_leave_the_gaps_alone(kind, layout):
    """n = 3 frames of 19 x 40 that are slices of bigger sentinel-filled buffers on both sides.  A base offset by 1 or 2 bytes, or a stride
    that is no multiple of 4, takes general; multiples of 4 stay on vec.  Every frame right and the same on both paths, every sentinel
    byte outside the frames untouched."""
    import torch
    from pythoncrt_amd import EgressYuv422, UnpackYuv422
    size, n = (19, 40), 3
    ybytes, rbytes = model.sizes(size[0], size[1], layout)[1], size[0] * size[1] * 3
    if kind == "unpack":
        src = model.sources(size[0], size[1], layout, n=n, seed=3)
        exp = _unpacked(src, size, layout).reshape(n, rbytes)
        sbytes, dbytes = ybytes, rbytes
    else:
        src = model.frames(*size, n=n, seed=3).reshape(n, rbytes)
        exp = _packed(src.reshape((n,) + size + (3,)), layout)
        sbytes, dbytes = rbytes, ybytes
    plan = (UnpackYuv422 if kind == "unpack" else EgressYuv422)(_dev(), size, layout)
    for s_off, d_off, s_pad, d_pad, vec in STRIDES:
        sbuf = torch.full((s_off + n * (sbytes + s_pad) + 16,), 0xEE, dtype=torch.uint8, device=_dev())
        dbuf = torch.full((d_off + n * (dbytes + d_pad) + 16,), 0x5A, dtype=torch.uint8, device=_dev())
        assert sbuf.data_ptr() % 4 == 0 and dbuf.data_ptr() % 4 == 0
        sview = sbuf[s_off:s_off + n * (sbytes + s_pad)].view(n, sbytes + s_pad)[:, :sbytes]
        dview = dbuf[d_off:d_off + n * (dbytes + d_pad)].view(n, dbytes + d_pad)[:, :dbytes]
        sview.copy_(torch.from_numpy(src).to(_dev()))
        if kind == "unpack":
            out = dview.unflatten(1, size + (3,))
            assert plan(sview, out=out) is out
        else:
            assert plan(sview.unflatten(1, size + (3,)), out=dview) is dview
        torch.cuda.synchronize()
        assert plan.last_plan() == _name(kind, layout, vec) + ";frames=3", (plan.last_plan(), s_off, d_off, s_pad, d_pad)
        assert np.array_equal(dview.cpu().numpy(), exp), (kind, layout, s_off, d_off, s_pad, d_pad)
        keep = torch.ones_like(dbuf, dtype=torch.bool)
        keep[d_off:d_off + n * (dbytes + d_pad)].view(n, dbytes + d_pad)[:, :dbytes] = False
        assert bool((dbuf[keep] == 0x5A).all()), (kind, layout, s_off, d_off)
    y, u, v = plan.planes(sview if kind == "unpack" else dview)
    assert tuple(y.shape) == (n,) + size and tuple(u.shape) == tuple(v.shape) == (n, size[0], size[1] // 2)
    plan.close()


# ---- bad arguments ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["unpack", "egress"])
def test_bad_arguments_return_the_stated_codes(kind):
    import torch
    from pythoncrt_amd import EgressYuv422, UnpackYuv422
    from pythoncrt_amd._lib import CrtfxError
    cls = UnpackYuv422 if kind == "unpack" else EgressYuv422
    with pytest.raises(CrtfxError) as e:
        cls(_dev(), (8, 8), "yuyv422", pix_fmt=_lib.PIX_F16)
    assert e.value.code == _lib.E_UNSUPPORTED and "uint8" in str(e.value)
    with pytest.raises(CrtfxError) as e:
        cls(_dev(), (0, 16), "yuyv422")
    assert e.value.code == _lib.E_INVALID
    with pytest.raises(ValueError):
        cls(_dev(), (8, 8), "nv12")
    with pytest.raises(ValueError):
        cls("cpu", (8, 8), "yuyv422")
    plan = cls(_dev(), (8, 8), "yuyv422")
    assert plan.frame_bytes == 128 and plan.last_plan() == _name(kind, "yuyv422", True) + ";frames=0"
    assert plan.plan() == {f"{kind}422": f"k_{kind}_422<yuyv422,vec>", "frames": "0"}
    plan.force_general = True
    assert plan.force_general and plan.last_plan() == _name(kind, "yuyv422", False) + ";frames=0"
    plan.force_general = False
    packed = torch.zeros((2, 128), dtype=torch.uint8, device=_dev())
    rgb = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=_dev())
    src, dst = (packed, rgb) if kind == "unpack" else (rgb, packed)
    sbytes, dbytes = (128, 192) if kind == "unpack" else (192, 128)
    with pytest.raises(CrtfxError) as e:
        plan(src.to(torch.float16))                                                             # a wrong dtype
    assert e.value.code == _lib.E_UNSUPPORTED
    with pytest.raises(ValueError):
        plan(src[:, :-2] if kind == "unpack" else src[:, :, :-1])                               # a wrong shape
    with pytest.raises(ValueError):
        plan(src, out=dst[:1])
    with pytest.raises(ValueError):
        plan(src.cpu())                                                                         # a wrong device
    with pytest.raises(ValueError):
        plan(src, out=dst.cpu())
    if kind == "egress":
        with pytest.raises(ValueError):
            plan(torch.zeros((2, 8, 16, 3), dtype=torch.uint8, device=_dev())[:, :, ::2])       # frames that are not contiguous
    assert int(plan(src[:0]).shape[0]) == 0                                                     # n == 0 is served
    with pytest.raises(CrtfxError) as e:
        plan.set_option(99, 1)
    assert e.value.code == _lib.E_INVALID and "option" in str(e.value)
    with pytest.raises(CrtfxError) as e:
        plan.set_option(1, 2)
    assert e.value.code == _lib.E_INVALID and "FORCE_GENERAL" in str(e.value)
    lib = plan.lib
    run, err = getattr(lib, f"crtfx_{kind}422_run"), getattr(lib, f"crtfx_{kind}422_last_error")
    st = torch.cuda.current_stream().cuda_stream
    dst.fill_(0)
    sp, dp = src.data_ptr(), dst.data_ptr()
    assert run(plan._plan, sp, sbytes, dp, dbytes, 0, st) == _lib.E_INVALID and b"n = 0" in err(plan._plan)
    assert run(plan._plan, None, sbytes, dp, dbytes, 1, st) == _lib.E_INVALID and b"null" in err(plan._plan)
    assert run(plan._plan, sp, sbytes, None, dbytes, 1, st) == _lib.E_INVALID
    assert run(plan._plan, sp, sbytes - 1, dp, dbytes, 2, st) == _lib.E_INVALID and b"strides" in err(plan._plan)  # a stride below a frame
    assert run(plan._plan, sp, sbytes, dp, dbytes - 1, 2, st) == _lib.E_INVALID and b"strides" in err(plan._plan)
    if torch.cuda.device_count() > 1:
        with torch.cuda.device(1 if _dev().index == 0 else 0):
            assert run(plan._plan, sp, sbytes, dp, dbytes, 1, st) == _lib.E_INVALID and b"current device" in err(plan._plan)
    torch.cuda.synchronize()
    assert int(dst.sum()) == 0                                                                  # no refused call wrote anything
    plan.close()


# ---- process_frames -----------------------------------------------------------------------------------------------------------------------

def _render_rgb24(frames, w, h, **kw):
    """What process_frames writes for rgb24 in and out: uint8 [n, h, w, 3]."""
    import pythoncrt_amd as pc
    got = []
    assert pc.process_frames(iter(frames), lambda a: got.append(np.array(a)), w, h, 30.0, len(frames), **kw) == len(frames)
    return np.stack(got)


def test_process_frames_takes_and_writes_422():
    """Five 36 x 64 frames in batches of 2, the grain fixed by noise_seed: yuv422p in -> nv12 out and rgb24 in -> yuyv422 out equal the
    models wrapped round the rgb24 run with the same seed; uyvy422 in -> uyvy422 out likewise (both ends, independently chosen)."""
    import pythoncrt_amd as pc
    h, w, n = 36, 64, 5
    kw = dict(noise_seed=9, batch=2, persistence=0.3)
    src = model.sources(h, w, "yuv422p", n=n, seed=44)
    rgb = _unpacked(src, (h, w), "yuv422p", "bt709", "pc")
    ref = _render_rgb24(rgb, w, h, **kw)
    got = []
    items = [src[0], src[1].reshape(2, -1)] + list(src[2:])                                   # any shape: it is flattened
    assert pc.process_frames(iter(items), lambda a: got.append(np.array(a)), w, h, 30.0, n, in_pix_fmt="yuv422p", in_matrix="bt709", in_range="pc",
                             out_pix_fmt="nv12", **kw) == n
    for i in range(n):
        exp = yuv_model.pack(ref[i], "nv12")
        assert got[i].shape == exp.shape and got[i].dtype == np.uint8 and np.array_equal(got[i], exp), ("yuv422p -> nv12", i)
    got = []
    assert pc.process_frames(iter(rgb), lambda a: got.append(np.array(a)), w, h, 30.0, n, out_pix_fmt="yuyv422", out_matrix="bt709", **kw) == n
    for i in range(n):
        exp = model.pack(ref[i], "yuyv422", "bt709", "tv")
        assert got[i].shape == exp.shape == (2 * h * w,) and np.array_equal(got[i], exp), ("rgb24 -> yuyv422", i)
    usrc = np.stack([model.relayout(p, h, w, "yuv422p", "uyvy422") for p in src])
    got = []
    assert pc.process_frames(pc.iter_yuv422(_Stream(usrc), w, h, "uyvy422"),
                             lambda a: got.append(np.array(a)), w, h, 30.0, n, in_pix_fmt="uyvy422", in_matrix="bt709", in_range="pc",
                             out_pix_fmt="uyvy422", **kw) == n
    for i in range(n):
        assert got[i].shape == usrc[i].shape and np.array_equal(got[i], model.pack(ref[i], "uyvy422")), ("uyvy422 -> uyvy422", i)
    with pytest.raises(ValueError) as e:                                                       # a 4:2:0 frame where a 4:2:2 one is due
        pc.process_frames(iter([np.zeros(h * w * 3 // 2, dtype=np.uint8)]), lambda a: None, w, h, 30.0, 1, in_pix_fmt="uyvy422")
    assert str(2 * h * w) in str(e.value)


def _Stream(frames):
    import io
    return io.BytesIO(np.ascontiguousarray(frames).tobytes())


def test_process_frames_resizes_an_off_size_422_source():
    """An 18 x 32 uyvy422 source for a 36 x 64 output: the frames go through IngestResize behind the source stage, and equal the rgb24 run
    fed the model's RGB with resize_on="device"."""
    import pythoncrt_amd as pc
    h, w, sh, sw, n = 36, 64, 18, 32, 3
    kw = dict(noise_seed=5, batch=2)
    src = model.sources(sh, sw, "uyvy422", n=n, seed=45)
    ref = _render_rgb24(_unpacked(src, (sh, sw), "uyvy422"), w, h, resize_on="device", **kw)
    got = []
    assert pc.process_frames(iter(src), lambda a: got.append(np.array(a)), w, h, 30.0, n, in_pix_fmt="uyvy422", in_size=(sh, sw), **kw) == n
    assert np.array_equal(np.stack(got), ref)


# ---- CLI ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("io", ["staged", "mapped"])
def test_cli_uyvy422_in_yuyv422_out(tmp_path, io):
    """--in-pix-fmt uyvy422 --out-pix-fmt yuyv422 over a 3-frame 36 x 64 file (batch 2: a full batch and a short one), --io staged and
    --io mapped: the output file equals pack(the rgb24 run of the same flags and seed on unpack(src))."""
    from pythoncrt_amd import cli
    n, h, w = 3, 36, 64
    src = model.sources(h, w, "uyvy422", n=n, seed=46)
    (tmp_path / "in.uyvy").write_bytes(src.tobytes())
    (tmp_path / "in.rgb").write_bytes(_unpacked(src, (h, w), "uyvy422", "bt709", "tv").tobytes())
    flags = ["--width", str(w), "--height", str(h), "--fps", "30", "--batch", "2", "--noise-seed", "17", "--persistence", "0.3", "--io", io]
    assert cli.main(flags + ["--input", str(tmp_path / "in.uyvy"), "--output", str(tmp_path / "out.yuyv"), "--in-pix-fmt", "uyvy422", "--in-matrix", "bt709",
                             "--out-pix-fmt", "yuyv422", "--out-range", "pc"]) == 0
    assert cli.main(flags + ["--input", str(tmp_path / "in.rgb"), "--output", str(tmp_path / "out.rgb")]) == 0
    got = np.frombuffer((tmp_path / "out.yuyv").read_bytes(), dtype=np.uint8)
    ref = np.frombuffer((tmp_path / "out.rgb").read_bytes(), dtype=np.uint8).reshape(n, h, w, 3)
    assert got.size == n * 2 * h * w
    _same(got.reshape(n, -1), _packed(ref, "yuyv422", "bt601", "pc"), io)
    assert not np.array_equal(ref[0], ref[1])
