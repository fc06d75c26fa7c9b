"""Resample filters in the render loop on the GPU: process_frames(in_filter=, deliver_filter=) and the CLI's --in-filter / --deliver-filter.
With another filter than "bilinear", Resample (include/crtfx_resample.h) stands where IngestResize / ResizeHalf stand.  8-bit delivery: the
frames written equal Pillow's resize, with that filter, of the frames the same call writes without deliver_size (and the 8-bit egress models
of those).  10-bit delivery: the models of the 10-bit stages around resample_model.resize_half of a half FramePipeline's output.  Source
side: the call equals its own run fed Pillow-resized frames, on the device and with resize_on="host".  "bilinear" is the path as it was."""
import numpy as np
import pytest

from pythoncrt_amd import formats
from tests import deep444_model, deep_model, egress_sited_model, unpack_model, yuv_model
from tests import resample_model as model

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


# ---- delivery, 8-bit ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filter", ["lanczos", "bicubic", "box"])
@pytest.mark.parametrize("size,deliver", PAIRS, ids=_ids)
def test_rgb24_frames_are_pillows_filtered_resize_of_the_rendered_frames(size, deliver, filter):
    base = _rendered(size)
    got = _render(_rgb_frames(size), size, deliver_size=deliver, deliver_filter=filter)
    for i, (a, b) in enumerate(zip(got, base)):
        exp = model.pillow(b, deliver[0], deliver[1], filter)
        assert a.shape == deliver + (3,) and a.dtype == np.uint8
        assert np.array_equal(a, exp), (size, deliver, filter, i, int((a != exp).sum()))
    if filter == "lanczos":                                        # ... and it is another picture than BILINEAR's
        assert not np.array_equal(got[0], _render(_rgb_frames(size), size, deliver_size=deliver)[0])


@pytest.mark.parametrize("fmt,chroma", [("yuv420p", "center"), ("yuv420p", "left")], ids=lambda v: str(v))
@pytest.mark.parametrize("size,deliver", PAIRS, ids=_ids)
def test_yuv_frames_are_the_egress_models_of_the_lanczos_frames(size, deliver, fmt, chroma):
    base = _rendered(size)
    got = _render(_rgb_frames(size), size, deliver_size=deliver, deliver_filter="lanczos", out_pix_fmt=fmt, out_matrix="bt709", out_range="pc",
                  out_chroma=chroma)
    fb = formats.frame_bytes(deliver[0], deliver[1], fmt)
    for i, (a, b) in enumerate(zip(got, base)):
        rgb = model.pillow(b, deliver[0], deliver[1], "lanczos")
        exp = egress_sited_model.pack(rgb, fmt, "left", "bt709", "pc") if chroma == "left" else yuv_model.pack(rgb, fmt, "bt709", "pc")
        assert a.shape == (fb,) and a.dtype == np.uint8
        assert np.array_equal(a, exp), (size, deliver, fmt, chroma, i, int((a != exp).sum()))


# ---- delivery, 10-bit -----------------------------------------------------------------------------------------------------------------------

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
def test_ten_bit_frames_are_the_models_of_the_lanczos_half_frames(size, deliver, in_fmt, out_fmt):
    """Three frames in two batches with persistence on.  Expected: pack(resample_model.resize_half(half FramePipeline output, "lanczos")) — the
    state stays at render size."""
    src, halves = _deep_case(in_fmt, size)
    got = _render(list(src), size, deliver_size=deliver, deliver_filter="lanczos", in_pix_fmt=in_fmt, out_pix_fmt=out_fmt)
    rendered = _half_render(halves, size)
    fb = formats.frame_bytes(deliver[0], deliver[1], out_fmt)
    for i in range(len(src)):
        exp = _pack10(model.resize_half(rendered[i], deliver[0], deliver[1], "lanczos"), out_fmt)
        assert got[i].shape == (fb,) and got[i].dtype == np.uint8
        assert np.array_equal(got[i], exp), (size, deliver, in_fmt, out_fmt, i, int((got[i] != exp).sum()))


# ---- the source side ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("src_size", [(23, 40), (67, 123)], ids=_ids)
def test_an_off_size_rgb24_source_is_resized_as_pillow_bicubic_does(src_size):
    """in_filter="bicubic" with frames of another size than the 46 x 80 output: the call equals its own run fed Pillow's BICUBIC resize of
    them, with the resize on the device and with resize_on="host"."""
    size = (46, 80)
    frames = _rgb_frames(src_size)
    want = _render([model.pillow(f, size[0], size[1], "bicubic") for f in frames], size)
    got = _render(frames, size, in_filter="bicubic")
    host = _render(frames, size, in_filter="bicubic", resize_on="host")
    for i in range(N):
        assert np.array_equal(got[i], want[i]), (src_size, i, int((got[i] != want[i]).sum()))
        assert np.array_equal(host[i], want[i]), (src_size, i)
    assert not np.array_equal(got[0], _render(frames, size)[0])             # ... and it is another picture than BILINEAR's


def test_an_off_size_yuv420p_source_is_resized_as_pillow_bicubic_does():
    """in_size = (18, 32) against a 36 x 64 output, in_filter="bicubic": the frames equal the rgb24 call fed Pillow's BICUBIC resize of the
    unpack model's 18 x 32 RGB."""
    size = (36, 64)
    rng = np.random.default_rng(42)
    fb = unpack_model.sizes(18, 32)[2]
    packed = [rng.integers(0, 256, fb, dtype=np.uint8) for _ in range(N)]
    want = _render([model.pillow(unpack_model.unpack(p, 18, 32, "yuv420p"), size[0], size[1], "bicubic") for p in packed], size)
    got = _render(packed, size, in_pix_fmt="yuv420p", in_size=(18, 32), in_filter="bicubic")
    for i in range(N):
        assert np.array_equal(got[i], want[i]), (i, int((got[i] != want[i]).sum()))


# ---- nothing changes without it -------------------------------------------------------------------------------------------------------------

def test_bilinear_passed_explicitly_is_the_default_and_builds_no_resample(monkeypatch):
    from pythoncrt_amd import resample

    def refuse(self, *a, **k):
        raise AssertionError("Resample was created")
    size, deliver = PAIRS[0]
    frames, small = _rgb_frames(size), _rgb_frames(deliver)
    src, _ = _deep_case("p010le", size)
    base = _render(frames, size, deliver_size=deliver)
    base_in = _render(small, size)
    base10 = _render(list(src), size, deliver_size=deliver, in_pix_fmt="p010le", out_pix_fmt="yuv420p10le")
    monkeypatch.setattr(resample.Resample, "__init__", refuse)
    same = _render(frames, size, deliver_size=deliver, deliver_filter="bilinear", in_filter="bilinear")
    assert all(np.array_equal(a, b) for a, b in zip(same, base))
    same = _render(small, size, in_filter="bilinear")
    assert all(np.array_equal(a, b) for a, b in zip(same, base_in))
    same = _render(list(src), size, deliver_size=deliver, deliver_filter="bilinear", in_pix_fmt="p010le", out_pix_fmt="yuv420p10le")
    assert all(np.array_equal(a, b) for a, b in zip(same, base10))
    with pytest.raises(AssertionError, match="Resample was created"):
        _render(frames, size, deliver_size=deliver, deliver_filter="hamming")
    with pytest.raises(AssertionError, match="Resample was created"):
        _render(small, size, in_filter="hamming")


# ---- CLI ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("io", ["staged", "mapped"])
@pytest.mark.parametrize("in_fmt,out_fmt", [("rgb24", "nv12"), ("p010le", "yuv420p10le")])
def test_cli_writes_what_process_frames_writes(tmp_path, io, in_fmt, out_fmt):
    """--deliver-filter lanczos --in-filter bicubic with --io staged and --io mapped, an 8-bit and a 10-bit case: the output file is N frames
    of frame_bytes(dh, dw, fmt) bytes, the bytes process_frames(deliver_filter="lanczos") hands to its writer for the same frames, settings and
    seed (a raw input file is read at render size: --in-filter has nothing to resize and changes nothing)."""
    from pythoncrt_amd import cli
    size, deliver = PAIRS[0]
    items = _rgb_frames(size) if in_fmt == "rgb24" else list(_deep_case(in_fmt, size, n=N)[0])
    (tmp_path / "in.raw").write_bytes(b"".join(np.ascontiguousarray(a).tobytes() for a in items))
    flags = ["--width", str(size[1]), "--height", str(size[0]), "--fps", "30", "--batch", str(BATCH), "--noise-seed", str(SEED), "--persistence", "0.35",
             "--pixel-size", "1", "--io", io, "--deliver-width", str(deliver[1]), "--deliver-height", str(deliver[0]), "--deliver-filter", "lanczos",
             "--in-filter", "bicubic", "--in-pix-fmt", in_fmt, "--out-pix-fmt", out_fmt]
    assert cli.main(flags + ["--input", str(tmp_path / "in.raw"), "--output", str(tmp_path / "out.raw")]) == 0
    fb = formats.frame_bytes(deliver[0], deliver[1], out_fmt)
    got = np.frombuffer((tmp_path / "out.raw").read_bytes(), dtype=np.uint8)
    assert got.size == N * fb, (got.size, N, fb)
    want = _render(items, size, deliver_size=deliver, deliver_filter="lanczos", in_pix_fmt=in_fmt, out_pix_fmt=out_fmt)
    other = _render(items, size, deliver_size=deliver, in_pix_fmt=in_fmt, out_pix_fmt=out_fmt)
    assert not np.array_equal(want[0], other[0])
    for i in range(N):
        assert np.array_equal(got.reshape(N, fb)[i], want[i].reshape(-1)), (io, in_fmt, i, int((got.reshape(N, fb)[i] != want[i].reshape(-1)).sum()))
