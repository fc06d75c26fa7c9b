"""process_frames(chain_pix="half", dither=) and the CLI's --chain-pix / --dither on the GPU: what the writer gets is the models' bytes —
the source model, tests/depth_model.widen, a half FramePipeline run by the test itself, the half geometry models, depth_model.narrow, the
egress model — composed in the order pythoncrt_amd/ends.py states.  5 frames in batches of 2 (the last one partial), the default
persistence carrying state across batches, the grain fixed by noise_seed.  Exact: there is no tolerance."""
import numpy as np
import pytest

from pythoncrt_amd import formats
from tests import canvas_model, deep444_model, deep_model, pil_resize_model, resize16_model, unpack_model, yuv422_model, yuv_model
from tests import depth_model as model

pytestmark = pytest.mark.gpu

N, BATCH, SEED = 5, 2, 23
SIZES = [(24, 136), (23, 131)]


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _frames(fmt, size, seed=0):
    """N frames of `fmt` as process_frames takes them: H x W x 3 for rgb24, else 1-D uint8 of frame_bytes; 10-bit samples are valid ones."""
    h, w = size
    rng = np.random.default_rng([h, w, seed, sum(map(ord, fmt))])
    nb = formats.frame_bytes(h, w, fmt)
    if fmt == "rgb24":
        return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(N)]
    if formats.bits(fmt) == 8:
        return [rng.integers(0, 256, nb, dtype=np.uint8) for _ in range(N)]
    shift = 6 if fmt == "p010le" else 0
    return [(rng.integers(0, 1024, nb // 2, dtype=np.uint16) << shift).astype("<u2").view(np.uint8) for _ in range(N)]


_PIPED = {}


def _pipe(frames_f16, size):
    """A half FramePipeline with process_frames' default settings over float16 [N, h, w, 3], in batches of BATCH with the state carried as
    the render loop carries it: float16 [N, h, w, 3]."""
    import torch
    from pythoncrt_amd.pipeline import FramePipeline, RenderSettings
    h, w = size
    x = torch.from_numpy(np.ascontiguousarray(frames_f16)).to(_dev())
    pipe = FramePipeline(_dev(), h, w, RenderSettings(), fps=30.0, noise_seed=SEED, dtype=torch.float16)
    outs, state = [], None
    for lo in range(0, N, BATCH):
        out, state = pipe.run(x[lo:lo + BATCH], first_index=lo, state=state)
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    res = np.concatenate(outs)
    assert res.dtype == np.float16 and res.shape == (N, h, w, 3)
    return res


def _rendered_rgb24(size):
    """pipe(widen(frames)) of the rgb24 frames of a size: computed once, shared by the tests that need it, never changed."""
    if size not in _PIPED:
        src = np.stack(_frames("rgb24", size))
        res = _pipe(model.widen(src), size)
        res.setflags(write=False)
        _PIPED[size] = res
    return _PIPED[size]


def _render(items, size, **kw):
    import pythoncrt_amd as pc
    got = []
    wrote = pc.process_frames(iter(items), lambda a: got.append(np.array(a)), size[1], size[0], 30.0, N, noise_seed=SEED, batch=BATCH, **kw)
    assert wrote == N == len(got) and all(a.dtype == np.uint8 for a in got)
    return got


def _check(got, exp, what):
    bad = [(i, int((np.asarray(g).reshape(-1) != np.asarray(e).reshape(-1)).sum())) for i, (g, e) in enumerate(zip(got, exp))
           if np.asarray(g).size != np.asarray(e).size or not np.array_equal(np.asarray(g).reshape(-1), np.asarray(e).reshape(-1))]
    assert len(got) == len(exp) and not bad, (what, bad)
    assert not np.array_equal(got[0], got[1])                                  # frames of a render, not one constant


@pytest.mark.parametrize("dither", model.DITHERS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rgb24_on_both_ends(size, dither):
    """narrow(pipe(widen(frames))): an rgb24 frame at render size goes through a source end whose only stage is the Widen, and the
    narrowed frames are what is downloaded."""
    got = _render(_frames("rgb24", size), size, chain_pix="half", dither=dither)
    assert all(a.shape == size + (3,) for a in got)
    _check(got, model.narrow(_rendered_rgb24(size), dither), ("rgb24", size, dither))
    if dither == "ordered":                                                    # the dither does something: the two roundings differ somewhere
        assert not np.array_equal(np.stack(got), model.narrow(_rendered_rgb24(size), "none"))


@pytest.mark.parametrize("dither", model.DITHERS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ten_bit_master_delivered_as_yuv420p(size, dither):
    h, w = size
    src = _frames("p010le", size)
    got = _render(src, size, chain_pix="half", dither=dither, in_pix_fmt="p010le", out_pix_fmt="yuv420p", out_matrix="bt709")
    rgb = np.stack([deep_model.unpack(p, h, w, "p010le") for p in src])
    u8 = model.narrow(_pipe(rgb, size), dither)
    _check(got, [yuv_model.pack(f, "yuv420p", "bt709") for f in u8], ("p010le", size, dither))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_eight_bit_sources_written_as_ten_bit(size):
    """nv12 at another size than the render (unpacked and resized on uint8 as ever, then widened) -> yuv420p10le, and uyvy422 -> x2rgb10le."""
    h, w = size
    sh, sw = 31, 90
    src = _frames("nv12", (sh, sw))
    got = _render(src, size, chain_pix="half", in_pix_fmt="nv12", in_size=(sh, sw), out_pix_fmt="yuv420p10le")
    rgb = np.stack([pil_resize_model.resize(unpack_model.unpack(p, sh, sw, "nv12"), h, w) for p in src])
    assert rgb.dtype == np.uint8
    _check(got, [deep_model.pack(f, "yuv420p10le") for f in _pipe(model.widen(rgb), size)], ("nv12", size))
    src = _frames("uyvy422", size)
    got = _render(src, size, chain_pix="half", in_pix_fmt="uyvy422", out_pix_fmt="x2rgb10le")
    rgb = np.stack([yuv422_model.unpack(p, h, w, "uyvy422") for p in src])
    _check(got, [deep444_model.pack(f, "x2rgb10le") for f in _pipe(model.widen(rgb), size)], ("uyvy422", size))


def _padded_nv12(size, deliver, color):
    """The delivery of test_narrowing_follows_the_half_geometry from the models: resize and pad on halves, then narrow, then nv12."""
    inner, at = canvas_model.fit_pad(size, deliver)
    assert inner != deliver and inner != size                                  # a resize and a Canvas stand in front of the Narrow
    half = resize16_model.resize(_rendered_rgb24(size), *inner)
    half = canvas_model.canvas(half, deliver, at=at, fill=np.array(color, dtype=np.float16))
    return [yuv_model.pack(f, "nv12") for f in model.narrow(half, "ordered")]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_narrowing_follows_the_half_geometry(size):
    """rgb24 -> nv12 with deliver_size, deliver_fit="pad" and the ordered dither: the resize and the Canvas run on the half frames, the Narrow
    at the delivery size behind them — its thresholds are those of the delivered frame's coordinates, bars included."""
    deliver, color = (36, 96), (7, 200, 33)
    got = _render(_frames("rgb24", size), size, chain_pix="half", dither="ordered", out_pix_fmt="nv12", deliver_size=deliver, deliver_fit="pad",
                  deliver_pad_color=color)
    _check(got, _padded_nv12(size, deliver, color), ("pad", size))


def test_resize_on_host_under_a_half_chain():
    """Off-size rgb24 frames resized by Pillow on the host, then widened on the device: the direct upload of `auto` is not taken."""
    size = SIZES[1]
    src = _frames("rgb24", (40, 75), seed=3)
    got = _render(src, size, chain_pix="half", dither="ordered", resize_on="host")
    rgb = np.stack([pil_resize_model.pillow(f, *size) for f in src])
    _check(got, model.narrow(_pipe(model.widen(rgb), size), "ordered"), "host")
    dev = _render(src, size, chain_pix="half", dither="ordered")               # ... and the device's resize gives the same bytes
    _check(dev, got, "device")


@pytest.fixture
def depth_plans(monkeypatch):
    """Counts the depth plans created, by class name."""
    from pythoncrt_amd import depth
    made = []
    for cls in (depth.Widen, depth.Narrow):
        def init(self, *a, _cls=cls, _init=cls.__init__, **kw):
            made.append(_cls.__name__)
            _init(self, *a, **kw)
        monkeypatch.setattr(cls, "__init__", init)
    return made


def test_auto_and_two_ten_bit_ends_build_no_depth_plan(depth_plans):
    size = SIZES[1]
    src = _frames("p010le", size)
    ten = dict(in_pix_fmt="p010le", out_pix_fmt="x2rgb10le")
    _check(_render(src, size, chain_pix="half", **ten), _render(src, size, chain_pix="auto", **ten), "10-bit on both ends")
    src = _frames("nv12", size)
    eight = dict(in_pix_fmt="nv12", out_pix_fmt="yuv420p")
    _check(_render(src, size, chain_pix="auto", dither="none", **eight), _render(src, size, **eight), "8-bit on both ends")
    assert depth_plans == []
    half = _render(src, size, chain_pix="half", **eight)
    assert depth_plans == ["Narrow", "Widen"]                                  # the delivery end is built first, one source end after it
    assert not np.array_equal(np.stack(half), np.stack(_render(src, size, **eight)))       # the half chain is another chain


CLI_CASES = [("p010le", "yuv420p", []), ("rgb24", "nv12", ["--deliver-height", "36", "--deliver-width", "96", "--deliver-fit", "pad", "--deliver-pad-color", "7,200,33"])]


@pytest.mark.parametrize("io", ["staged", "mapped"])
@pytest.mark.parametrize("case", CLI_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_cli_writes_what_process_frames_hands_its_writer(tmp_path, case, io):
    from pythoncrt_amd import cli
    in_fmt, out_fmt, extra = case
    size = SIZES[1]
    h, w = size
    items = _frames(in_fmt, size)
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    src.write_bytes(b"".join(a.tobytes() for a in items))
    assert cli.main(["--input", str(src), "--output", str(dst), "--width", str(w), "--height", str(h), "--fps", "30", "--batch", str(BATCH),
                     "--noise-seed", str(SEED), "--in-pix-fmt", in_fmt, "--out-pix-fmt", out_fmt, "--chain-pix", "half", "--dither", "ordered",
                     "--io", io] + extra) == 0
    kw = dict(deliver_size=(36, 96), deliver_fit="pad", deliver_pad_color=(7, 200, 33)) if extra else {}
    got = _render(items, size, chain_pix="half", dither="ordered", in_pix_fmt=in_fmt, out_pix_fmt=out_fmt, **kw)
    fb = formats.frame_bytes(*((36, 96) if extra else size), out_fmt)
    written = np.frombuffer(dst.read_bytes(), dtype=np.uint8)
    assert written.size == N * fb, (written.size, N, fb)
    _check([written[i * fb:(i + 1) * fb] for i in range(N)], got, (case, io))
    if extra:                                                                  # ... which are the models' bytes
        _check(got, _padded_nv12(size, (36, 96), (7, 200, 33)), "pad")
