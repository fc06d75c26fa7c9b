"""process_frames(in_signal=, signal_standard="pal", pal_decoder=, signal_phase=) and the CLI's --signal-standard / --pal-decoder /
--signal-phase on the GPU: what the writer gets is the models' bytes — the source model, tests/pal_model at the SOURCE's size with t
counting source frames over the WHOLE sequence, [tests/deint_model], [the resize model], [widen], a FramePipeline run by the test itself
over the whole sequence, [the egress model] — composed in the order pythoncrt_amd/ends.py states.  The chain's batches are smaller than the
sequence.  Exact: there is no tolerance."""
import numpy as np
import pytest

from tests import deep444_model, deep_model, deint_model, depth_model, field420_model, pil_resize_model, yuv422_model
from tests import pal_model as model
from tests import signal_model
from tests.test_signal_pipeline_gpu import N, SD, SEED, SIZE, _check, _frames, _pipe, _render

pytestmark = pytest.mark.gpu

PAL = dict(in_signal="composite", signal_standard="pal")


@pytest.mark.parametrize("signal,chroma,crawl,decoder,phase", [("composite", "sharp", True, "delay", 0), ("svideo", "soft", True, "simple", -20),
                                                                ("composite", "soft", False, "delay", 20)])
def test_rgb24_at_render_size(signal, chroma, crawl, decoder, phase):
    """The PalSignal is the source end's only stage; batches of 2 and 3 over 5 frames: the index runs on across them, mod 4."""
    src = _frames("rgb24", SIZE)
    cable = model.pal(np.stack(src), signal, chroma, crawl, 0, decoder, phase)
    kw = dict(in_signal=signal, signal_standard="pal", signal_chroma=chroma, signal_crawl=crawl, pal_decoder=decoder, signal_phase=phase)
    _check(_render(src, SIZE, N, batch=2, **kw), _pipe(cable, SIZE, 2), ("rgb24", signal, chroma, crawl, decoder, phase))
    _check(_render(src, SIZE, N, batch=3, **kw), _pipe(cable, SIZE, 3), "odd batches: the second starts at t = 3")
    if signal == "composite" and crawl:
        restarted = np.concatenate([model.pal(np.stack(src[lo:lo + 3]), signal, chroma, True, 0, decoder, phase) for lo in (0, 3)])
        assert not np.array_equal(restarted, cable)                            # a count that began again per batch would be other frames
        assert not np.array_equal(cable, signal_model.signal(np.stack(src), signal, chroma, True, 0))      # and PAL is not NTSC


def test_interlaced_yuv420p_deinterlaced_to_both_fields():
    """576i 4:2:0's path: UnpackField420, the PalSignal on the woven frame, then the Deinterlace; t counts SOURCE frames."""
    h, w = SIZE
    src = _frames("yuv420p", SIZE)
    rgb = np.stack([field420_model.unpack(p, h, w, "yuv420p", "replicate") for p in src])
    cable = model.pal(rgb, "composite", "sharp", True, 0, "delay", 0)
    fields = deint_model.deinterlace(cable, "edge", "tff", "both")
    got = _render(src, SIZE, 2 * N, batch=4, in_pix_fmt="yuv420p", in_chroma_rows="interlaced", deinterlace="edge", deinterlace_fields="both", **PAL)
    _check(got, _pipe(fields, SIZE, 4), "yuv420p interlaced edge both")
    got = _render(src, SIZE, 2 * N, batch=2, in_pix_fmt="yuv420p", in_chroma_rows="interlaced", deinterlace="edge", deinterlace_fields="both", **PAL)
    _check(got, _pipe(fields, SIZE, 2), "batches of ONE source frame: t = 0, 1, 2, 3, 4")


def test_p010le_on_the_half_chain():
    h, w = SIZE
    src = _frames("p010le", SIZE)
    rgb = np.stack([deep_model.unpack(p, h, w, "p010le") for p in src])
    assert rgb.dtype == np.float16
    exp = _pipe(model.pal(rgb, "composite", "soft", True, 0, "delay", 20), SIZE, 2)
    got = _render(src, SIZE, N, batch=2, in_pix_fmt="p010le", out_pix_fmt="yuv444p10le", signal_chroma="soft", signal_phase=20, **PAL)
    _check(got, [deep444_model.pack(f, "yuv444p10le") for f in exp], "p010le pal")


def test_chain_pix_half_with_the_simple_decoder_and_a_phase_error():
    """chain_pix="half" with an rgb24 source: the PalSignal runs on uint8 frames in front of the Widen."""
    src = _frames("rgb24", SIZE, seed=2)
    cable = model.pal(np.stack(src), "composite", "sharp", True, 0, "simple", 20)
    exp = depth_model.narrow(_pipe(depth_model.widen(cable), SIZE, 2))
    _check(_render(src, SIZE, N, batch=2, chain_pix="half", pal_decoder="simple", signal_phase=20, **PAL), exp, "half chain")
    assert not np.array_equal(cable, model.pal(np.stack(src), "composite", "sharp", True, 0, "delay", 20))


def test_a_mixed_size_stream_keeps_counting_mod_4():
    """rgb24 frames of two sizes, batch 4: [a a a] t = 0, 1, 2; [b] t = 3 — at ITS size, by another source end; [a a a] t = 4, 5, 6."""
    h, w = SIZE
    a, b = _frames("rgb24", SIZE, seed=4), _frames("rgb24", SD, seed=5)
    src = [a[0], a[1], a[2], b[0], a[3], a[4], a[0]]
    cable = [model.pal(f[None], "composite", "sharp", True, t, "delay", 0)[0] for t, f in enumerate(src)]
    rgb = np.stack([f if f.shape[:2] == SIZE else pil_resize_model.resize(f, h, w) for f in cable])
    _check(_render(src, SIZE, 7, batch=4, **PAL), _pipe(rgb, SIZE, [3, 1, 3]), "mixed sizes")
    assert not np.array_equal(model.pal(src[3][None], "composite", "sharp", True, 0, "delay", 0)[0], cable[3])       # a count per source end
    assert not np.array_equal(cable[6], cable[0]) and np.array_equal(model.pal(src[6][None], "composite", "sharp", True, 2, "delay", 0)[0], cable[6])


@pytest.fixture
def plans(monkeypatch):
    """Records the Signal and PalSignal plans created."""
    from pythoncrt_amd import pal, signal
    made = []
    for cls in (signal.Signal, pal.PalSignal):
        def init(self, *a, _cls=cls, _init=cls.__init__, **kw):
            made.append((_cls, a[1:], kw))
            _init(self, *a, **kw)
        monkeypatch.setattr(cls, "__init__", init)
    return made


def test_ntsc_gives_the_bytes_of_before_and_builds_no_pal_signal(plans):
    import torch
    from pythoncrt_amd import pal, signal
    src = _frames("rgb24", SIZE)
    before = _render(src, SIZE, N, batch=2, in_signal="composite", signal_chroma="soft")
    assert plans == [(signal.Signal, (SIZE,), {"signal": "composite", "chroma": "soft", "crawl": True, "dtype": torch.uint8})]
    del plans[:]
    _check(_render(src, SIZE, N, batch=2, in_signal="composite", signal_chroma="soft", signal_standard="ntsc", pal_decoder="delay", signal_phase=0), before, "ntsc")
    assert plans == [(signal.Signal, (SIZE,), {"signal": "composite", "chroma": "soft", "crawl": True, "dtype": torch.uint8})]
    _check(before, _pipe(signal_model.signal(np.stack(src), "composite", "soft", True, 0), SIZE, 2), "the NTSC cable as it was")
    del plans[:]
    plain = _render(src, SIZE, N, batch=2)
    _check(_render(src, SIZE, N, batch=2, signal_standard="ntsc"), plain, "no signal")
    _check(plain, _pipe(np.stack(src), SIZE, 2), "the chain as it was")
    assert plans == []
    _render(src, SIZE, N, batch=2, signal_chroma="soft", **PAL)
    assert plans == [(pal.PalSignal, (SIZE,), {"signal": "composite", "chroma": "soft", "crawl": True, "decoder": "delay", "phase": 0, "dtype": torch.uint8})]


@pytest.mark.parametrize("io", ["staged", "mapped"])
def test_cli_sends_the_input_through_the_pal_cable(tmp_path, io):
    """--signal-standard pal on both --io paths, batches of 2 over 5 frames, uyvy422 out: the bytes process_frames writes."""
    from pythoncrt_amd import cli
    h, w = SIZE
    items = _frames("rgb24", SIZE, seed=6)
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    src.write_bytes(b"".join(a.tobytes() for a in items))
    base = ["--input", str(src), "--output", str(dst), "--width", str(w), "--height", str(h), "--fps", "30", "--noise-seed", str(SEED), "--io", io]
    flags = ["--batch", "2", "--in-signal", "composite", "--signal-standard", "pal", "--signal-chroma", "soft", "--pal-decoder", "simple", "--signal-phase", "-20",
             "--out-pix-fmt", "uyvy422"]
    assert cli.main(base + flags) == 0
    exp = [yuv422_model.pack(f, "uyvy422") for f in _pipe(model.pal(np.stack(items), "composite", "soft", True, 0, "simple", -20), SIZE, 2)]
    fb = np.asarray(exp[0]).size
    written = np.frombuffer(dst.read_bytes(), dtype=np.uint8)
    assert written.size == N * fb, (written.size, fb)
    _check([written[i * fb:(i + 1) * fb] for i in range(N)], exp, io)
    same = _render(items, SIZE, N, batch=2, in_signal="composite", signal_standard="pal", signal_chroma="soft", pal_decoder="simple", signal_phase=-20,
                   out_pix_fmt="uyvy422")
    _check([written[i * fb:(i + 1) * fb] for i in range(N)], same, (io, "process_frames"))
