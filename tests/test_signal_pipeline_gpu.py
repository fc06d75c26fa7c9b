"""process_frames(in_signal=, signal_chroma=, signal_crawl=) and the CLI's --in-signal / --signal-chroma / --signal-crawl on the GPU: what the
writer gets is the models' bytes — the source model, tests/signal_model at the SOURCE's size with t counting source frames over the WHOLE
sequence, [tests/deint_model], [the resize model], [widen], a FramePipeline run by the test itself over the whole sequence, [the egress
model] — composed in the order pythoncrt_amd/ends.py states.  The chain's batches are smaller than the sequence, the default persistence
carries state across them, the grain is fixed by noise_seed.  Exact: there is no tolerance."""
import numpy as np
import pytest

from pythoncrt_amd import formats
from tests import deep444_model, deep_model, deint_model, depth_model, pil_resize_model, unpack_model, yuv422_model
from tests import signal_model as model

pytestmark = pytest.mark.gpu

N, SEED = 5, 31
SIZE = (24, 136)
SD = (18, 96)                           # an off-size source: the stage runs at THIS size, the resize behind it


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _frames(fmt, size, seed=0, n=N):
    """n frames of `fmt` as process_frames takes them: H x W x 3 for rgb24, else 1-D uint8 of frame_bytes; 10-bit samples are valid ones."""
    h, w = size
    rng = np.random.default_rng([h, w, seed, sum(map(ord, fmt))])
    nb = formats.frame_bytes(h, w, fmt)
    if fmt == "rgb24":
        return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)]
    if formats.bits(fmt) == 8:
        return [rng.integers(0, 256, nb, dtype=np.uint8) for _ in range(n)]
    shift = 6 if fmt == "p010le" else 0
    return [(rng.integers(0, 1024, nb // 2, dtype=np.uint16) << shift).astype("<u2").view(np.uint8) for _ in range(n)]


def _pipe(frames, size, batches):
    """A FramePipeline of the frames' dtype with process_frames' default settings over [n, h, w, 3], in batches of `batches` (an int, or the
    list of batch lengths) with the frame index running on and the state carried as the render loop carries it.  -> all output frames."""
    import torch
    from pythoncrt_amd.pipeline import FramePipeline, RenderSettings
    h, w = size
    x = torch.from_numpy(np.ascontiguousarray(frames)).to(_dev())
    if isinstance(batches, int):
        batches = [min(batches, x.shape[0] - lo) for lo in range(0, x.shape[0], batches)]
    assert sum(batches) == x.shape[0]
    pipe = FramePipeline(_dev(), h, w, RenderSettings(), fps=30.0, noise_seed=SEED, dtype=x.dtype)
    outs, state, lo = [], None, 0
    for b in batches:
        out, state = pipe.run(x[lo:lo + b], first_index=lo, state=state)
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
        lo += b
    return np.concatenate(outs)


def _render(items, size, n_out, **kw):
    import pythoncrt_amd as pc
    got = []
    wrote = pc.process_frames(iter(items), lambda a: got.append(np.array(a)), size[1], size[0], 30.0, n_out, noise_seed=SEED, **kw)
    assert wrote == n_out == len(got) and all(a.dtype == np.uint8 for a in got)
    return got


def _check(got, exp, what):
    bad = [(i, int((np.asarray(g).reshape(-1) != np.asarray(e).reshape(-1)).sum())) for i, (g, e) in enumerate(zip(got, exp))
           if np.asarray(g).size != np.asarray(e).size or not np.array_equal(np.asarray(g).reshape(-1), np.asarray(e).reshape(-1))]
    assert len(got) == len(exp) and not bad, (what, bad)
    assert not np.array_equal(got[0], got[1])                                  # frames of a render, not one constant


@pytest.mark.parametrize("signal,chroma,crawl", [("composite", "sharp", True), ("svideo", "soft", True), ("composite", "soft", False)])
def test_rgb24_at_render_size(signal, chroma, crawl):
    """The Signal is the source end's only stage; batches of 2 over 5 frames: frame 2 and 3 are t = 2, 3, not 0, 1."""
    src = _frames("rgb24", SIZE)
    cable = model.signal(np.stack(src), signal, chroma, crawl, 0)
    exp = _pipe(cable, SIZE, 2)
    kw = dict(in_signal=signal, signal_chroma=chroma, signal_crawl=crawl)
    _check(_render(src, SIZE, N, batch=2, **kw), exp, ("rgb24", signal, chroma, crawl))
    _check(_render(src, SIZE, N, batch=3, **kw), _pipe(cable, SIZE, 3), "odd batches: the second starts at t = 3")
    if signal == "composite" and crawl:
        restarted = np.concatenate([model.signal(np.stack(src[lo:lo + 3]), signal, chroma, True, 0) for lo in (0, 3)])
        assert not np.array_equal(restarted, cable)                            # a count that began again per batch would be other frames
        assert not np.array_equal(cable, np.stack(src))


def test_off_size_nv12_with_in_size():
    """nv12 at SD: the source plan, the Signal at SD, then the resize to the render size."""
    h, w = SD
    src = _frames("nv12", SD)
    rgb = np.stack([unpack_model.unpack(p, h, w, "nv12") for p in src])
    cable = model.signal(rgb, "composite", "soft", True, 0)
    exp = _pipe(np.stack([pil_resize_model.resize(f, *SIZE) for f in cable]), SIZE, 2)
    got = _render(src, SIZE, N, batch=2, in_pix_fmt="nv12", in_size=SD, in_signal="composite", signal_chroma="soft")
    _check(got, exp, "nv12 at SD")
    late = model.signal(np.stack([pil_resize_model.resize(f, *SIZE) for f in rgb]), "composite", "soft", True, 0)
    assert not np.array_equal(_pipe(late, SIZE, 2), exp)                       # the stage behind the resize is another picture


def test_uyvy422_deinterlaced_to_both_fields():
    """The cable carried the fields: the Signal in front of the Deinterlace, t counting SOURCE frames while the chain counts fields."""
    h, w = SIZE
    src = _frames("uyvy422", SIZE)
    rgb = np.stack([yuv422_model.unpack(p, h, w, "uyvy422") for p in src])
    cable = model.signal(rgb, "composite", "sharp", True, 0)
    fields = deint_model.deinterlace(cable, "edge", "tff", "both")
    exp = _pipe(fields, SIZE, 4)
    got = _render(src, SIZE, 2 * N, batch=4, in_pix_fmt="uyvy422", deinterlace="edge", deinterlace_fields="both", in_signal="composite")
    _check(got, exp, "uyvy422 edge both")
    counted_in_fields = np.concatenate([model.signal(rgb[lo:lo + 2], "composite", "sharp", True, 2 * lo) for lo in (0, 2, 4)])
    assert np.array_equal(counted_in_fields, cable)                            # batches of 2 source frames start at even t either way ...
    got = _render(src, SIZE, 2 * N, batch=2, in_pix_fmt="uyvy422", deinterlace="edge", deinterlace_fields="both", in_signal="composite")
    _check(got, _pipe(fields, SIZE, 2), "... batches of ONE source frame do not: t = 0, 1, 2, 3, 4, not the chain's 0, 2, 4, 6, 8")


def test_p010le_on_the_half_chain():
    h, w = SIZE
    src = _frames("p010le", SIZE)
    rgb = np.stack([deep_model.unpack(p, h, w, "p010le") for p in src])
    assert rgb.dtype == np.float16
    exp = _pipe(model.signal(rgb, "svideo", "sharp", True, 0), SIZE, 2)
    got = _render(src, SIZE, N, batch=2, in_pix_fmt="p010le", out_pix_fmt="yuv444p10le", in_signal="svideo")
    _check(got, [deep444_model.pack(f, "yuv444p10le") for f in exp], "p010le svideo")


def test_chain_pix_half_keeps_the_signal_on_the_sources_bytes():
    """chain_pix="half" with an rgb24 source: the Signal runs on uint8 frames in front of the Widen."""
    src = _frames("rgb24", SIZE, seed=2)
    cable = model.signal(np.stack(src), "composite", "soft", False, 0)
    exp = depth_model.narrow(_pipe(depth_model.widen(cable), SIZE, 2))
    _check(_render(src, SIZE, N, batch=2, chain_pix="half", in_signal="composite", signal_chroma="soft", signal_crawl=False), exp, "half chain")


def test_a_mixed_size_stream_keeps_counting():
    """rgb24 frames of two sizes, batch 4: [a a a] t = 0, 1, 2; [b] t = 3 — at ITS size, by another source end; [a a] t = 4, 5."""
    h, w = SIZE
    a, b = _frames("rgb24", SIZE, seed=4), _frames("rgb24", SD, seed=5)
    src = [a[0], a[1], a[2], b[0], a[3], a[4]]
    cable = [model.signal(f[None], "composite", "sharp", True, t)[0] for t, f in enumerate(src)]
    rgb = np.stack([f if f.shape[:2] == SIZE else pil_resize_model.resize(f, h, w) for f in cable])
    exp = _pipe(rgb, SIZE, [3, 1, 2])
    _check(_render(src, SIZE, 6, batch=4, in_signal="composite"), exp, "mixed sizes")
    assert not np.array_equal(model.signal(src[3][None], "composite", "sharp", True, 0)[0], cable[3])      # a count per source end would be another frame


@pytest.fixture
def signal_plans(monkeypatch):
    """Records the Signal plans created."""
    from pythoncrt_amd import signal
    made = []
    init0 = signal.Signal.__init__

    def init(self, *a, **kw):
        made.append((a[1:], kw))
        init0(self, *a, **kw)
    monkeypatch.setattr(signal.Signal, "__init__", init)
    return made


def test_rgb_builds_no_signal_and_gives_the_bytes_of_before(signal_plans):
    import torch
    src = _frames("rgb24", SIZE)
    plain = _render(src, SIZE, N, batch=2)
    _check(_render(src, SIZE, N, batch=2, in_signal="rgb", signal_chroma="sharp", signal_crawl=True), plain, "rgb")
    _check(plain, _pipe(np.stack(src), SIZE, 2), "the chain as it was")
    _render(_frames("nv12", SD), SIZE, N, batch=2, in_pix_fmt="nv12", in_size=SD, chain_pix="half", out_pix_fmt="uyvy422")
    assert signal_plans == []
    _render(_frames("nv12", SD), SIZE, N, batch=2, in_pix_fmt="nv12", in_size=SD, chain_pix="half", in_signal="svideo", signal_chroma="soft")
    assert signal_plans == [((SD,), {"signal": "svideo", "chroma": "soft", "crawl": True, "dtype": torch.uint8})]


@pytest.mark.parametrize("io", ["staged", "mapped"])
def test_cli_sends_the_input_through_the_cable(tmp_path, io):
    """--in-signal on both --io paths, batches of 2 over 5 frames, uyvy422 out."""
    from pythoncrt_amd import cli
    h, w = SIZE
    items = _frames("rgb24", SIZE, seed=6)
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    src.write_bytes(b"".join(a.tobytes() for a in items))
    base = ["--input", str(src), "--output", str(dst), "--width", str(w), "--height", str(h), "--fps", "30", "--noise-seed", str(SEED), "--io", io]
    assert cli.main(base + ["--batch", "2", "--in-signal", "composite", "--signal-chroma", "soft", "--out-pix-fmt", "uyvy422"]) == 0
    exp = [yuv422_model.pack(f, "uyvy422") for f in _pipe(model.signal(np.stack(items), "composite", "soft", True, 0), SIZE, 2)]
    fb = np.asarray(exp[0]).size
    written = np.frombuffer(dst.read_bytes(), dtype=np.uint8)
    assert written.size == N * fb, (written.size, fb)
    _check([written[i * fb:(i + 1) * fb] for i in range(N)], exp, io)
    assert cli.main(base + ["--batch", "2", "--in-signal", "composite", "--signal-chroma", "soft", "--signal-crawl", "off", "--out-pix-fmt", "uyvy422"]) == 0
    still = [yuv422_model.pack(f, "uyvy422") for f in _pipe(model.signal(np.stack(items), "composite", "soft", False, 0), SIZE, 2)]
    written = np.frombuffer(dst.read_bytes(), dtype=np.uint8)
    _check([written[i * fb:(i + 1) * fb] for i in range(N)], still, (io, "crawl off"))
    assert not np.array_equal(np.stack(still), np.stack(exp))
