"""Frame geometry through process_frames and the CLI: deliver_fit="pad" / "crop" behind the chain and in_crop in front of it.  Delivery:
the bytes written equal the numpy model's pad / crop (tests/canvas_model.py) around Pillow's resize (uint8) or resize16_model's (half) of
the frames the same call renders without delivery flags, through the egress models.  Source: a run with in_crop equals a run fed the
pre-cropped frames.  The helpers, settings and seed are those of tests/test_deliver_gpu.py."""
import numpy as np
import pytest

from pythoncrt_amd import formats
from tests import canvas_model as model
from tests import deep_model, pil_resize_model, resample_model, resize16_model, unpack_model
from tests import test_deliver_gpu as dl

pytestmark = pytest.mark.gpu

FILL = (7, 200, 33)
# render size -> delivery size.  4:3 into 16:9: pad = resize to 27 x 36 then bars of 6 columns, crop = rows 3..21 resized up; a wide odd
# render into a tall delivery: pad = resize to 17 x 30 then bars of 7 rows, crop = columns 9..31 resized
PAIRS = [((24, 32), (27, 48)), ((23, 41), (31, 30))]
N = dl.N


def _ids(p):
    return f"{p[0]}x{p[1]}"


def _pad_u8(frame, deliver, filter="bilinear"):
    inner, at = model.fit_pad(frame.shape[:2], deliver)
    small = frame if inner == frame.shape[:2] else resample_model.pillow(frame, inner[0], inner[1], filter)
    return model.canvas(small, deliver, at=at, fill=FILL)


def _crop_u8(frame, deliver):
    win = model.fit_crop(frame.shape[:2], deliver)
    cut = model.crop(frame, win)
    return cut if win[2:] == tuple(deliver) else pil_resize_model.pillow(cut, *deliver)


def test_the_pairs_take_every_stage():
    assert [model.fit_pad(s, d) for s, d in PAIRS] == [((27, 36), (0, 6)), ((17, 30), (7, 0))]
    assert [model.fit_crop(s, d) for s, d in PAIRS] == [(3, 0, 18, 32), (0, 9, 23, 22)]


@pytest.mark.parametrize("fmt,chroma", [("rgb24", "center"), ("nv12", "center"), ("uyvy422", "left")], ids=lambda v: str(v))
@pytest.mark.parametrize("fit", ["pad", "crop"])
@pytest.mark.parametrize("size,deliver", PAIRS, ids=_ids)
def test_eight_bit_delivery(size, deliver, fit, fmt, chroma):
    base = dl._rendered(size)                                                   # the same call without delivery flags, same frames and seed
    kw = dict(out_pix_fmt=fmt, out_matrix="bt709", out_range="pc", out_chroma=chroma) if fmt != "rgb24" else {}
    got = dl._render(dl._rgb_frames(size), size, deliver_size=deliver, deliver_fit=fit, deliver_pad_color=FILL, **kw)
    for i, (a, b) in enumerate(zip(got, base)):
        rgb = _pad_u8(b, deliver) if fit == "pad" else _crop_u8(b, deliver)
        assert rgb.shape == deliver + (3,)
        exp = rgb if fmt == "rgb24" else dl._pack8(rgb, fmt, chroma)
        assert a.shape == exp.shape and a.dtype == np.uint8
        assert np.array_equal(a, exp), (size, deliver, fit, fmt, i, int((a != exp).sum()))


@pytest.mark.parametrize("fit,deliver", [("pad", (24, 40)), ("crop", (18, 32))])
def test_a_fit_that_needs_no_resize(fit, deliver, monkeypatch):
    """24 x 32 padded to 24 x 40 and cut to 18 x 32: the inner frame / the window has its final size, and no resize plan is created."""
    from pythoncrt_amd import ingest
    size = (24, 32)
    base = dl._rendered(size)

    def refuse(self, *a, **k):
        raise AssertionError("IngestResize was created")
    monkeypatch.setattr(ingest.IngestResize, "__init__", refuse)
    got = dl._render(dl._rgb_frames(size), size, deliver_size=deliver, deliver_fit=fit, deliver_pad_color=FILL)
    for i, (a, b) in enumerate(zip(got, base)):
        exp = model.canvas(b, deliver, at=(0, 4), fill=FILL) if fit == "pad" else model.crop(b, (3, 0, 18, 32))
        assert np.array_equal(a, exp), (fit, i, int((a != exp).sum()))


def test_pad_with_a_lanczos_resize():
    size, deliver = PAIRS[0]
    base = dl._rendered(size)
    got = dl._render(dl._rgb_frames(size), size, deliver_size=deliver, deliver_fit="pad", deliver_pad_color=FILL, deliver_filter="lanczos")
    for i, (a, b) in enumerate(zip(got, base)):
        exp = _pad_u8(b, deliver, "lanczos")
        assert np.array_equal(a, exp), (i, int((a != exp).sum()))
    assert not np.array_equal(got[0], _pad_u8(base[0], deliver))                # another picture than BILINEAR's


@pytest.mark.parametrize("fit", ["pad", "crop"])
@pytest.mark.parametrize("size,deliver", PAIRS, ids=_ids)
def test_ten_bit_delivery(size, deliver, fit):
    """p010le -> p010le, three frames in two batches with persistence on.  The render-size half frames are a half FramePipeline's with the
    call's settings and seed (the construction of tests/test_deliver_gpu.py), tied to the call by its run without delivery flags."""
    src, halves = dl._deep_case("p010le", size)
    rendered = dl._half_render(halves, size)
    plain = dl._render(list(src), size, in_pix_fmt="p010le", out_pix_fmt="p010le")
    got = dl._render(list(src), size, deliver_size=deliver, deliver_fit=fit, deliver_pad_color=FILL, in_pix_fmt="p010le", out_pix_fmt="p010le")
    fb = formats.frame_bytes(deliver[0], deliver[1], "p010le")
    for i in range(len(src)):
        assert np.array_equal(plain[i], deep_model.pack(rendered[i], "p010le")), i
        if fit == "pad":
            inner, at = model.fit_pad(size, deliver)
            rgb = model.canvas(resize16_model.resize(rendered[i], *inner), deliver, at=at, fill=np.array(FILL, dtype=np.float16))
        else:
            rgb = resize16_model.resize(model.crop(rendered[i], model.fit_crop(size, deliver)), *deliver)
        exp = deep_model.pack(rgb, "p010le")
        assert got[i].shape == (fb,) and np.array_equal(got[i], exp), (size, deliver, fit, i, int((got[i] != exp).sum()))


def test_same_aspect_pad_and_crop_are_stretch():
    size = (24, 32)
    for deliver in ((12, 16), (36, 48)):
        want = dl._render(dl._rgb_frames(size), size, deliver_size=deliver, out_pix_fmt="nv12")
        for fit in ("pad", "crop"):
            got = dl._render(dl._rgb_frames(size), size, deliver_size=deliver, deliver_fit=fit, deliver_pad_color=FILL, out_pix_fmt="nv12")
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (deliver, fit)


# ---- in_crop ------------------------------------------------------------------------------------------------------------------------------------

def test_in_crop_on_rgb24_frames_of_mixed_sizes():
    """Frames of 30 x 44, of the render size itself and of 40 x 50, the size changing inside and between batches: the run equals a run
    fed the windows themselves."""
    size, crop = (24, 32), (3, 5, 20, 26)
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((30, 44), (30, 44), (24, 32), (40, 50), (40, 50), (24, 32), (30, 44))]
    want = dl._render([model.crop(f, crop) for f in frames], size)
    got = dl._render(frames, size, in_crop=crop)
    for i in range(len(frames)):
        assert np.array_equal(got[i], want[i]), (i, int((got[i] != want[i]).sum()))
    assert not np.array_equal(got[2], dl._render(frames[2:3], size)[0])          # a render-size frame is cropped too
    with pytest.raises(ValueError, match="in_crop.*22 x 40"):
        dl._render([np.zeros((22, 40, 3), dtype=np.uint8)], size, in_crop=crop)


def test_in_crop_on_an_nv12_source_with_in_size():
    size, in_size, crop = (23, 41), (30, 44), (2, 3, 25, 38)
    rng = np.random.default_rng(4)
    fb = unpack_model.sizes(*in_size)[2]
    packed = [rng.integers(0, 256, fb, dtype=np.uint8) for _ in range(N)]
    rgb = [unpack_model.unpack(p, in_size[0], in_size[1], "nv12", "bt709", "pc") for p in packed]
    want = dl._render([model.crop(f, crop) for f in rgb], size)
    got = dl._render(packed, size, in_pix_fmt="nv12", in_matrix="bt709", in_range="pc", in_size=in_size, in_crop=crop)
    for i in range(N):
        assert np.array_equal(got[i], want[i]), (i, int((got[i] != want[i]).sum()))


def test_in_crop_on_a_p010le_source_whose_window_is_the_render_size():
    """A 28 x 40 p010le source, window (2, 4, 24, 32) = the render size: the Canvas runs in half in front of the half chain.  With even
    offsets the window of the source's RGB is the RGB of the window's own planes (asserted on the model), so the run must equal a run fed
    those planes as 24 x 32 p010le frames."""
    size, in_size, crop = (24, 32), (28, 40), (2, 4, 24, 32)
    src, halves = dl._deep_case("p010le", in_size)
    small = []
    for p, rgb in zip(src, halves):
        y, u, v = deep_model.planes(p, in_size[0], in_size[1], "p010le")
        cut = deep_model.pack_planes(y[2:26, 4:36], u[1:13, 2:18], v[1:13, 2:18], "p010le")
        assert np.array_equal(deep_model.unpack(cut, 24, 32, "p010le").view(np.uint16), model.crop(rgb, crop).view(np.uint16))
        small.append(cut)
    want = dl._render(small, size, in_pix_fmt="p010le", out_pix_fmt="p010le")
    got = dl._render(list(src), size, in_pix_fmt="p010le", out_pix_fmt="p010le", in_size=in_size, in_crop=crop)
    for i in range(len(src)):
        assert np.array_equal(got[i], want[i]), (i, int((got[i] != want[i]).sum()))


# ---- nothing changes without it -----------------------------------------------------------------------------------------------------------------

def test_the_defaults_create_no_canvas(monkeypatch):
    import torch
    from pythoncrt_amd import canvas, ends
    dev = dl._dev()
    for deliver in (None, (12, 16), (27, 48)):
        end = ends.DeliveryEnd(dev, (24, 32), torch.uint8, "nv12", "bt601", "tv", "center", deliver, "bilinear")
        assert end.canvas is None and (end.resize is None) == (deliver is None) and len(end.stages) == (deliver is not None)
    src = ends.SourceEnd(dev, (24, 32), "nv12", "bt601", "tv", "replicate", (30, 44), "bilinear")
    assert src.canvas is None and src.resize is not None and len(src.stages) == 2
    end = ends.DeliveryEnd(dev, (24, 32), torch.uint8, "rgb24", "bt601", "tv", "center", (27, 48), "bilinear", deliver_fit="pad", pad_color=FILL)
    assert isinstance(end.canvas, canvas.Canvas) and end.canvas.fill == FILL and end.canvas.at == (0, 6) and len(end.stages) == 2

    def refuse(self, *a, **k):
        raise AssertionError("Canvas was created")
    monkeypatch.setattr(canvas.Canvas, "__init__", refuse)
    size = (24, 32)
    base = dl._rendered(size)
    got = dl._render(dl._rgb_frames(size), size, in_crop=None, deliver_fit="stretch", deliver_pad_color=(0, 0, 0))
    assert all(np.array_equal(a, b) for a, b in zip(got, base))
    dl._render(dl._rgb_frames((30, 44)), size, deliver_size=(27, 48), out_pix_fmt="nv12")
    with pytest.raises(AssertionError, match="Canvas was created"):
        dl._render(dl._rgb_frames(size), size, deliver_size=(27, 48), deliver_fit="pad")


# ---- CLI ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("io", ["staged", "mapped"])
@pytest.mark.parametrize("in_fmt,out_fmt,fit", [("rgb24", "nv12", "pad"), ("nv12", "rgb24", "crop")])
def test_cli_writes_what_process_frames_writes(tmp_path, io, in_fmt, out_fmt, fit):
    """--in-crop-*, --deliver-fit and --deliver-pad-color with --io staged and --io mapped: the output file is N frames of the DELIVERY
    size, the bytes process_frames hands to its writer for the same frames, settings and seed."""
    from pythoncrt_amd import cli
    size, deliver = PAIRS[0]
    crop = (2, 4, 18, 24)
    if in_fmt == "rgb24":
        items = dl._rgb_frames(size)
    else:
        rng = np.random.default_rng(9)
        items = [rng.integers(0, 256, formats.frame_bytes(size[0], size[1], in_fmt), dtype=np.uint8) for _ in range(N)]
    (tmp_path / "in.raw").write_bytes(b"".join(np.ascontiguousarray(a).tobytes() for a in items))
    flags = dl._cli_flags(size, deliver, io, ["--in-pix-fmt", in_fmt, "--out-pix-fmt", out_fmt, "--deliver-fit", fit, "--deliver-pad-color", "7,200,33",
                                              "--in-crop-y", "2", "--in-crop-x", "4", "--in-crop-height", "18", "--in-crop-width", "24"])
    assert cli.main(flags + ["--input", str(tmp_path / "in.raw"), "--output", str(tmp_path / "out.raw")]) == 0
    fb = formats.frame_bytes(deliver[0], deliver[1], out_fmt)
    got = np.frombuffer((tmp_path / "out.raw").read_bytes(), dtype=np.uint8)
    assert got.size == N * fb, (got.size, N, fb)
    want = dl._render(items, size, deliver_size=deliver, deliver_fit=fit, deliver_pad_color=FILL, in_crop=crop, in_pix_fmt=in_fmt, out_pix_fmt=out_fmt)
    plain = dl._render(items, size, deliver_size=deliver, in_pix_fmt=in_fmt, out_pix_fmt=out_fmt)
    assert not np.array_equal(want[0], plain[0])                               # the flags do something
    for i in range(N):
        assert np.array_equal(got.reshape(N, fb)[i], want[i].reshape(-1)), (io, in_fmt, i, int((got.reshape(N, fb)[i] != want[i].reshape(-1)).sum()))
