"""Delivery size on the GPU: process_frames(deliver_size=) and the CLI's --deliver-width / --deliver-height.  The chain renders at
out_h x out_w; behind it the finished frames are resized on the device (IngestResize for uint8 frames, ResizeHalf for half ones) and the
egress plan, the download and the writer see the delivery size.  8-bit: the frames written equal Pillow's BILINEAR resize of the frames the
same call writes without deliver_size (and the 8-bit egress models of those).  10-bit: the models of the 10-bit egress stages applied to
resize16_model.resize of a half FramePipeline's output, the construction tests/test_deep_gpu.py uses around the chain."""
import numpy as np
import pytest

from pythoncrt_amd import formats
from tests import deep444_model, deep_model, egress_sited_model, pil_resize_model, resize16_model, yuv422_model, yuv_model

pytestmark = pytest.mark.gpu

PAIRS = [((46, 80), (23, 40)), ((45, 80), (67, 123))]            # render size -> delivery size: 1/2 with an odd delivery height; a ragged up-scale
KW = dict(persistence=0.35, pixel_size=1)                         # persistence on: a wrong state frame would corrupt every later frame
N, BATCH, SEED = 5, 2, 31                                         # three batches, the last one short


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _ids(p):
    return f"{p[0]}x{p[1]}"


def _rgb_frames(size, n=N, seed=0):
    rng = np.random.default_rng([seed, size[0], size[1]])
    return [rng.integers(0, 256, size + (3,), dtype=np.uint8) for _ in range(n)]


def _render(items, size, n=None, **kw):
    import pythoncrt_amd as pc
    got = []
    args = dict(KW)
    args.update(kw)
    wrote = pc.process_frames(iter(items), lambda a: got.append(np.array(a)), size[1], size[0], 30.0, n or len(items), noise_seed=SEED, batch=BATCH, **args)
    assert wrote == len(items) == len(got)
    return got


_RENDERED = {}


def _rendered(size):
    """The rgb24 frames process_frames writes at render size, without deliver_size: rendered once per size, left unchanged."""
    if size not in _RENDERED:
        out = _render(_rgb_frames(size), size)
        assert all(a.shape == size + (3,) and a.dtype == np.uint8 for a in out) and not np.array_equal(out[0], out[1])
        for a in out:
            a.setflags(write=False)
        _RENDERED[size] = out
    return _RENDERED[size]


# ---- 8-bit ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size,deliver", PAIRS, ids=_ids)
def test_rgb24_frames_are_pillows_resize_of_the_rendered_frames(size, deliver):
    base = _rendered(size)
    got = _render(_rgb_frames(size), size, deliver_size=deliver)
    for i, (a, b) in enumerate(zip(got, base)):
        exp = pil_resize_model.pillow(b, *deliver)
        assert a.shape == deliver + (3,) and a.dtype == np.uint8
        assert np.array_equal(a, exp), (size, deliver, i, int((a != exp).sum()))


def _pack8(rgb, fmt, chroma):
    if chroma == "left":
        return egress_sited_model.pack(rgb, fmt, "left", "bt709", "pc")
    if fmt in yuv422_model.LAYOUTS:
        return yuv422_model.pack(rgb, fmt, "bt709", "pc")
    return yuv_model.pack(rgb, fmt, "bt709", "pc")


@pytest.mark.parametrize("fmt,chroma", [("yuv420p", "center"), ("nv12", "center"), ("uyvy422", "center"), ("yuv420p", "left"), ("uyvy422", "left")],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("size,deliver", PAIRS, ids=_ids)
def test_yuv_frames_are_the_egress_models_of_the_resized_frames(size, deliver, fmt, chroma):
    """The box stages (yuv_model, yuv422_model) and the sited stage (egress_sited_model) are built for the delivery size and read the
    resized frames: the bytes written are the models' of Pillow's resize of the rendered rgb24 frames."""
    base = _rendered(size)
    got = _render(_rgb_frames(size), size, deliver_size=deliver, out_pix_fmt=fmt, out_matrix="bt709", out_range="pc", out_chroma=chroma)
    fb = formats.frame_bytes(deliver[0], deliver[1], fmt)
    for i, (a, b) in enumerate(zip(got, base)):
        exp = _pack8(pil_resize_model.pillow(b, *deliver), fmt, chroma)
        assert a.shape == (fb,) and a.dtype == np.uint8
        assert np.array_equal(a, exp), (size, deliver, fmt, chroma, i, int((a != exp).sum()))


# ---- 10-bit ---------------------------------------------------------------------------------------------------------------------------------

def _half_render(rgb_half, size, n_batch=BATCH):
    """A half FramePipeline with process_frames's settings and seed over float16 [n, h, w, 3], in batches with the state carried, as the render
    loops do: float16 [n, h, w, 3] at RENDER size."""
    import torch
    from pythoncrt_amd.pipeline import FramePipeline, RenderSettings
    pipe = FramePipeline(_dev(), size[0], size[1], RenderSettings(**KW), fps=30.0, noise_seed=SEED, dtype=torch.float16)
    src = torch.from_numpy(rgb_half.view(np.int16)).to(_dev()).view(torch.float16)
    outs, state = [], None
    for lo in range(0, len(rgb_half), n_batch):
        out, state = pipe.run(src[lo:lo + n_batch], first_index=lo, state=state)
        torch.cuda.synchronize()
        outs.append(out.view(torch.int16).cpu().numpy().view(np.float16))
    return np.concatenate(outs)


def _deep_case(in_fmt, size, n=3):
    """(packed source frames uint8 [n, frame_bytes], the model's halves of them)"""
    fb = formats.frame_bytes(size[0], size[1], in_fmt)
    words = np.random.default_rng([7, size[0], size[1]]).integers(0, 1024, (n, fb // 2)).astype(np.uint16)
    if in_fmt == "p010le":
        src = deep_model.to_bytes(words << 6).reshape(n, fb)
        return src, np.stack([deep_model.unpack(p, size[0], size[1], in_fmt) for p in src])
    src = deep_model.to_bytes(words).reshape(n, fb)
    return src, np.stack([deep444_model.unpack(p, size[0], size[1], in_fmt) for p in src])


def _pack10(half, fmt):
    return deep_model.pack(half, fmt) if fmt in deep_model.LAYOUTS else deep444_model.pack(half, fmt)


@pytest.mark.parametrize("in_fmt,out_fmt", [("p010le", "p010le"), ("yuv444p10le", "x2rgb10le")])
@pytest.mark.parametrize("size,deliver", PAIRS, ids=_ids)
def test_ten_bit_frames_are_the_models_of_the_resized_half_frames(size, deliver, in_fmt, out_fmt):
    """Three frames in two batches with persistence on.  Expected: pack(resize16_model.resize(half FramePipeline output)) — the state stays at
    render size (a state kept at delivery size, or a resize in front of the chain, would give other bytes from the second frame on)."""
    src, halves = _deep_case(in_fmt, size)
    got = _render(list(src), size, deliver_size=deliver, in_pix_fmt=in_fmt, out_pix_fmt=out_fmt)
    rendered = _half_render(halves, size)
    fb = formats.frame_bytes(deliver[0], deliver[1], out_fmt)
    for i in range(len(src)):
        exp = _pack10(resize16_model.resize(rendered[i], *deliver), out_fmt)
        assert got[i].shape == (fb,) and got[i].dtype == np.uint8
        assert np.array_equal(got[i], exp), (size, deliver, in_fmt, out_fmt, i, int((got[i] != exp).sum()))
    plain = _render(list(src), size, in_pix_fmt=in_fmt, out_pix_fmt=out_fmt)            # ... and without deliver_size: the rendered frames themselves
    for i in range(len(src)):
        assert np.array_equal(plain[i], _pack10(rendered[i], out_fmt)), (in_fmt, out_fmt, i)


# ---- nothing changes without it ------------------------------------------------------------------------------------------------------------

def test_render_size_and_none_are_the_path_as_it_was(monkeypatch):
    """deliver_size=None and deliver_size == (out_h, out_w): the same bytes, and neither a ResizeHalf nor an IngestResize plan is created."""
    from pythoncrt_amd import ingest, resize16

    def refuse(self, *a, **k):
        raise AssertionError(f"{type(self).__name__} was created")
    monkeypatch.setattr(ingest.IngestResize, "__init__", refuse)
    monkeypatch.setattr(resize16.ResizeHalf, "__init__", refuse)
    size = PAIRS[0][0]
    base = _rendered(size) if size in _RENDERED else _render(_rgb_frames(size), size)
    for kw in (dict(deliver_size=None), dict(deliver_size=size), dict(deliver_size=list(size))):
        got = _render(_rgb_frames(size), size, **kw)
        assert all(np.array_equal(a, b) for a, b in zip(got, base)), kw
    nv = _render(_rgb_frames(size), size, out_pix_fmt="nv12")
    assert all(np.array_equal(a, b) for a, b in zip(_render(_rgb_frames(size), size, out_pix_fmt="nv12", deliver_size=size), nv))
    src, _ = _deep_case("p010le", size)
    plain = _render(list(src), size, in_pix_fmt="p010le", out_pix_fmt="yuv420p10le")
    same = _render(list(src), size, in_pix_fmt="p010le", out_pix_fmt="yuv420p10le", deliver_size=size)
    assert all(np.array_equal(a, b) for a, b in zip(plain, same))
    with pytest.raises(AssertionError, match="IngestResize was created"):
        _render(_rgb_frames(size), size, deliver_size=PAIRS[0][1])


# ---- CLI ------------------------------------------------------------------------------------------------------------------------------------

def _cli_flags(size, deliver, io, extra):
    return ["--width", str(size[1]), "--height", str(size[0]), "--fps", "30", "--batch", str(BATCH), "--noise-seed", str(SEED), "--persistence", "0.35",
            "--pixel-size", "1", "--io", io, "--deliver-width", str(deliver[1]), "--deliver-height", str(deliver[0])] + extra


@pytest.mark.parametrize("io", ["staged", "mapped"])
@pytest.mark.parametrize("in_fmt,out_fmt", [("rgb24", "nv12"), ("p010le", "yuv420p10le")])
def test_cli_writes_what_process_frames_writes(tmp_path, io, in_fmt, out_fmt):
    """--deliver-width / --deliver-height with --io staged and --io mapped, an 8-bit and a 10-bit case: the output file is N frames of
    frame_bytes(dh, dw, fmt) bytes, the bytes process_frames(deliver_size=) hands to its writer for the same frames, settings and seed."""
    from pythoncrt_amd import cli
    size, deliver = PAIRS[0]
    if in_fmt == "rgb24":
        items = _rgb_frames(size)
    else:
        items = list(_deep_case(in_fmt, size, n=N)[0])
    (tmp_path / "in.raw").write_bytes(b"".join(np.ascontiguousarray(a).tobytes() for a in items))
    flags = _cli_flags(size, deliver, io, ["--in-pix-fmt", in_fmt, "--out-pix-fmt", out_fmt, "--staging-report"])
    assert cli.main(flags + ["--input", str(tmp_path / "in.raw"), "--output", str(tmp_path / "out.raw")]) == 0
    fb = formats.frame_bytes(deliver[0], deliver[1], out_fmt)
    got = np.frombuffer((tmp_path / "out.raw").read_bytes(), dtype=np.uint8)
    assert got.size == N * fb, (got.size, N, fb)
    want = _render(items, size, deliver_size=deliver, in_pix_fmt=in_fmt, out_pix_fmt=out_fmt)
    for i in range(N):
        assert np.array_equal(got.reshape(N, fb)[i], want[i].reshape(-1)), (io, in_fmt, i, int((got.reshape(N, fb)[i] != want[i].reshape(-1)).sum()))


@pytest.mark.parametrize("io", ["staged", "mapped"])
def test_cli_failed_render_is_cut_back_to_whole_delivery_frames(tmp_path, monkeypatch, io):
    """A file-to-file render over an existing longer output that dies in its third batch: the file holds whole frames of the DELIVERY size,
    a prefix of the good render, for the growing staged output and for the pre-sized mapped one."""
    from pythoncrt_amd import cli
    from pythoncrt_amd.pipeline import FramePipeline
    size, deliver = PAIRS[0]
    n = 9
    fb = deliver[0] * deliver[1] * 3
    src, dst = tmp_path / "in.rgb", tmp_path / "out.rgb"
    src.write_bytes(b"".join(a.tobytes() for a in _rgb_frames(size, n=n)))
    flags = _cli_flags(size, deliver, io, ["--input", str(src), "--output", str(dst)])
    assert cli.main(flags) == 0
    good = dst.read_bytes()
    assert len(good) == n * fb
    dst.write_bytes(b"\xaa" * ((n + 6) * size[0] * size[1] * 3))          # an earlier, longer render at render size
    real, calls = FramePipeline.run, [0]

    def run(self, *a, **k):
        calls[0] += 1
        if calls[0] == 3:
            raise RuntimeError("injected failure in batch 3")
        return real(self, *a, **k)
    monkeypatch.setattr(FramePipeline, "run", run)
    with pytest.raises(RuntimeError, match="injected failure"):
        cli.main(flags)
    monkeypatch.undo()
    left = dst.read_bytes()
    assert len(left) % fb == 0 and len(left) <= 2 * BATCH * fb, (io, len(left), fb)
    assert left == good[:len(left)]
    assert cli.main(flags) == 0 and dst.read_bytes() == good
