"""process_frames(deliver_interlace=, deliver_lowpass=) and the CLI's --deliver-interlace / --deliver-lowpass on the GPU: what the writer gets
is the models' bytes — [the source model, tests/deint_model], [widen], a FramePipeline run by the test itself over the whole sequence, [the
delivery resize and Canvas models], tests/interlace_model at the DELIVERY size, [narrow], the egress model — composed in the order
pythoncrt_amd/ends.py states.  The chain's batches are smaller than the sequence, the default persistence carries state across them, the
grain is fixed by noise_seed.  Exact: there is no tolerance."""
import numpy as np
import pytest

from pythoncrt_amd import formats
from tests import canvas_model, deep444_model, deep_model, deint_model, depth_model, pil_resize_model, resize16_model, yuv422_model
from tests import interlace_model as model

pytestmark = pytest.mark.gpu

N, SEED = 5, 31
SIZE = (24, 136)


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
    list of batch lengths) with the frame index running on and the state carried as the render loop carries it.  -> the list of the
    batches' outputs."""
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
    return outs


def _weave(outs, order, lowpass, between=lambda f: f):
    """The delivery of the chain's batches: `between` (the delivery geometry) on each, then the Interlace per BATCH — pairs never straddle one."""
    return np.concatenate([model.interlace(between(o), order, lowpass) for o in outs])


def _render(items, size, n_out, **kw):
    import pythoncrt_amd as pc
    got, progress = [], []
    wrote = pc.process_frames(iter(items), lambda a: got.append(np.array(a)), size[1], size[0], 30.0, n_out, noise_seed=SEED,
                              progress_cb=progress.append, **kw)
    assert wrote == n_out == len(got) and all(a.dtype == np.uint8 for a in got)      # the return value and `written`: DELIVERED frames
    assert progress == [(i + 1) / n_out for i in range(n_out)]                  # ... and so does progress_cb, against total_frames as such
    return got


def _check(got, exp, what):
    bad = [(i, int((np.asarray(g).reshape(-1) != np.asarray(e).reshape(-1)).sum())) for i, (g, e) in enumerate(zip(got, exp))
           if np.asarray(g).size != np.asarray(e).size or not np.array_equal(np.asarray(g).reshape(-1), np.asarray(e).reshape(-1))]
    assert len(got) == len(exp) and not bad, (what, bad)
    assert not np.array_equal(got[0], got[1])                                  # frames of a render, not one constant


def test_rgb24_field_rate_chain_delivered_interlaced():
    """rgb24, deinterlace="edge" to both fields, deliver_interlace="tff": N frames in, 2 N through the chain in batches of 4, N out."""
    src = _frames("rgb24", SIZE)
    fields = deint_model.deinterlace(np.stack(src), "edge", "tff", "both")
    outs = _pipe(fields, SIZE, 4)
    assert [len(o) for o in outs] == [4, 4, 2]
    exp = _weave(outs, "tff", "none")
    got = _render(src, SIZE, N, batch=4, deinterlace="edge", deinterlace_fields="both", deliver_interlace="tff")
    assert all(a.shape == SIZE + (3,) for a in got)
    _check(got, exp, "rgb24 edge both tff")
    _check(_render(src, SIZE, N, batch=5, deinterlace="edge", deinterlace_fields="both", deliver_interlace="tff"), exp, "batch=5 is taken as 4")
    assert not np.array_equal(np.stack(got), _weave(outs, "bff", "none"))      # the order matters


def test_uyvy422_out_with_bff_and_linear():
    src = _frames("rgb24", SIZE, seed=1)
    fields = deint_model.deinterlace(np.stack(src), "linear", "bff", "both")
    exp = _weave(_pipe(fields, SIZE, 4), "bff", "linear")
    got = _render(src, SIZE, N, batch=4, deinterlace="linear", field_order="bff", deinterlace_fields="both", out_pix_fmt="uyvy422",
                  deliver_interlace="bff", deliver_lowpass="linear")
    _check(got, [yuv422_model.pack(f, "uyvy422") for f in exp], "uyvy422 bff linear")


def test_half_chain_low_pass_in_front_of_the_dithered_narrow_on_a_padded_delivery():
    """chain_pix="half", dither="ordered", deliver_size with deliver_fit="pad": resize and Canvas on halves, the Interlace at the DELIVERY size
    on halves, then the Narrow with the delivered frame's coordinates — not the Narrow first and the low-pass on bytes."""
    deliver, color = (36, 96), (7, 200, 33)
    inner, at = canvas_model.fit_pad(SIZE, deliver)
    assert inner != deliver and inner != SIZE
    src = _frames("rgb24", SIZE, seed=2)
    fields = deint_model.deinterlace(np.stack(src), "linear", "tff", "both")
    outs = _pipe(depth_model.widen(fields), SIZE, 4)

    def geometry(f):
        return canvas_model.canvas(resize16_model.resize(f, *inner), deliver, at=at, fill=np.array(color, dtype=np.float16))
    exp = depth_model.narrow(_weave(outs, "tff", "linear", geometry), "ordered")
    got = _render(src, SIZE, N, batch=4, deinterlace="linear", deinterlace_fields="both", chain_pix="half", dither="ordered", deliver_size=deliver,
                  deliver_fit="pad", deliver_pad_color=color, deliver_interlace="tff", deliver_lowpass="linear")
    assert all(a.shape == deliver + (3,) for a in got)
    _check(got, exp, "half, pad, ordered, linear")
    late = _weave([depth_model.narrow(geometry(o), "ordered") for o in outs], "tff", "linear")
    assert not np.array_equal(late, exp)                                       # the other order of the two stages is another picture


def test_p010le_to_yuv444p10le_with_complex():
    h, w = SIZE
    src = _frames("p010le", SIZE)
    rgb = np.stack([deep_model.unpack(p, h, w, "p010le") for p in src])
    fields = deint_model.deinterlace(rgb, "edge", "tff", "both")
    exp = _weave(_pipe(fields, SIZE, 4), "tff", "complex")
    got = _render(src, SIZE, N, batch=4, deinterlace="edge", deinterlace_fields="both", in_pix_fmt="p010le", out_pix_fmt="yuv444p10le",
                  deliver_interlace="tff", deliver_lowpass="complex")
    _check(got, [deep444_model.pack(f, "yuv444p10le") for f in exp], "p010le -> yuv444p10le complex")


@pytest.mark.parametrize("batch,lens", [(2, [2, 2, 1]), (4, [4, 1]), (3, [2, 2, 1]), (1, [2, 2, 1])])
def test_a_progressive_source_of_five_frames_gives_three(batch, lens):
    """No deinterlacer: 5 frames through the chain, 3 delivered, the last one woven with itself; the batch is taken even and at least 2."""
    src = _frames("rgb24", SIZE, seed=3)
    outs = _pipe(np.stack(src), SIZE, lens)
    exp = _weave(outs, "bff", "linear")
    assert exp.shape[0] == 3 and np.array_equal(exp[2], model.filtered(outs[-1][-1], "linear"))
    _check(_render(src, SIZE, 3, batch=batch, deliver_interlace="bff", deliver_lowpass="linear"), exp, ("progressive", batch))


def test_a_mixed_size_stream_cuts_a_batch_at_an_odd_count():
    """rgb24 frames of two sizes without a deinterlacer, batch 4: [a a a] is cut by the change of size and its third frame is woven with
    itself, [b b] is one pair, [a] is woven with itself: 6 frames in, 4 out."""
    h, w = SIZE
    a, b = _frames("rgb24", SIZE, seed=4), _frames("rgb24", (31, 90), seed=5)
    src = [a[0], a[1], a[2], b[0], b[1], a[3]]
    rgb = np.stack([f if f.shape[:2] == SIZE else pil_resize_model.resize(f, h, w) for f in src])
    outs = _pipe(rgb, SIZE, [3, 2, 1])
    exp = _weave(outs, "tff", "complex")
    assert exp.shape[0] == 4
    _check(_render(src, SIZE, 4, batch=4, deliver_interlace="tff", deliver_lowpass="complex"), exp, "mixed sizes")
    assert not np.array_equal(exp, model.interlace(np.concatenate(outs), "tff", "complex"))      # pairs across the cut would be other frames


@pytest.fixture
def interlace_plans(monkeypatch):
    """Records the Interlace plans created."""
    from pythoncrt_amd import interlace
    made = []
    init0 = interlace.Interlace.__init__

    def init(self, *a, **kw):
        made.append((a[1:], kw))
        init0(self, *a, **kw)
    monkeypatch.setattr(interlace.Interlace, "__init__", init)
    return made


def test_off_builds_no_interlace_and_gives_the_bytes_of_before(interlace_plans):
    import torch
    src = _frames("rgb24", SIZE)
    plain = _render(src, SIZE, N, batch=2)
    _check(_render(src, SIZE, N, batch=2, deliver_interlace="off", deliver_lowpass="none"), plain, "off")
    _check(plain, np.concatenate(_pipe(np.stack(src), SIZE, 2)), "the chain as it was")
    _check(_render(src, SIZE, N, batch=3), np.concatenate(_pipe(np.stack(src), SIZE, 3)), "an odd batch stays odd")
    _render(_frames("nv12", (31, 90)), SIZE, N, batch=2, in_pix_fmt="nv12", in_size=(31, 90), chain_pix="half", out_pix_fmt="uyvy422",
            deliver_size=(36, 96), deliver_fit="pad")
    assert interlace_plans == []
    _render(src, SIZE, 3, batch=2, deliver_interlace="bff", deliver_size=(36, 96), chain_pix="half")
    assert interlace_plans == [(((36, 96),), {"order": "bff", "lowpass": "none", "dtype": torch.float16})]


@pytest.mark.parametrize("io", ["staged", "mapped"])
@pytest.mark.parametrize("case", ["progressive", "field-rate"])
def test_cli_writes_ceil_n_over_two_delivery_frames(tmp_path, case, io):
    """The file holds ceil(N / 2) delivery frames (N under --deinterlace-fields both) and the model's bytes, sized from the delivered count."""
    from pythoncrt_amd import cli
    h, w = SIZE
    items = _frames("rgb24", SIZE, seed=6)
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    src.write_bytes(b"".join(a.tobytes() for a in items))
    dst.write_bytes(bytes(7 * h * w * 3))                                       # a longer file of an earlier render: cut back to the delivered frames
    base = ["--input", str(src), "--output", str(dst), "--width", str(w), "--height", str(h), "--fps", "30", "--noise-seed", str(SEED), "--io", io]
    if case == "progressive":
        assert cli.main(base + ["--batch", "2", "--deliver-interlace", "bff", "--deliver-lowpass", "complex"]) == 0
        exp = list(_weave(_pipe(np.stack(items), SIZE, 2), "bff", "complex"))
        n_out = 3
    else:
        assert cli.main(base + ["--batch", "4", "--deinterlace", "linear", "--deinterlace-fields", "both", "--out-pix-fmt", "uyvy422",
                                "--deliver-interlace", "tff", "--deliver-lowpass", "linear"]) == 0
        fields = deint_model.deinterlace(np.stack(items), "linear", "tff", "both")
        exp = [yuv422_model.pack(f, "uyvy422") for f in _weave(_pipe(fields, SIZE, 4), "tff", "linear")]
        n_out = N
    fb = np.asarray(exp[0]).size
    written = np.frombuffer(dst.read_bytes(), dtype=np.uint8)
    assert written.size == n_out * fb, (written.size, n_out, fb)
    _check([written[i * fb:(i + 1) * fb] for i in range(n_out)], exp, (case, io))
