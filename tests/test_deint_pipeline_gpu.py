"""process_frames(deinterlace=, field_order=, deinterlace_fields=) and the CLI's --deinterlace flags on the GPU: what the writer gets is
the models' bytes — the source model, tests/deint_model at the SOURCE size, the crop, the resize model, [widen], a FramePipeline run by the
test itself, [narrow], the egress model — composed in the order pythoncrt_amd/ends.py states.  5 source frames; under "first" in batches
of 2, under "both" 10 frames in chain batches of 4 (the last one partial either way), the default persistence carrying state across
batches, the grain fixed by noise_seed.  Exact: there is no tolerance."""
import numpy as np
import pytest

from pythoncrt_amd import formats
from tests import deep_model, depth_model, pil_resize_model, unpack_model, yuv422_model
from tests import deint_model as model

pytestmark = pytest.mark.gpu

N, SEED = 5, 29
SIZE = (24, 136)
BATCH = {"first": 2, "both": 4}         # the chain's batch: under "both" two source frames feed it


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


def _pipe(frames, size, batch):
    """A FramePipeline of the frames' dtype with process_frames' default settings over [n, h, w, 3], in batches of `batch` with the frame
    index running on and the state carried as the render loop carries it."""
    import torch
    from pythoncrt_amd.pipeline import FramePipeline, RenderSettings
    h, w = size
    x = torch.from_numpy(np.ascontiguousarray(frames)).to(_dev())
    pipe = FramePipeline(_dev(), h, w, RenderSettings(), fps=30.0, noise_seed=SEED, dtype=x.dtype)
    outs, state = [], None
    for lo in range(0, x.shape[0], batch):
        out, state = pipe.run(x[lo:lo + batch], first_index=lo, state=state)
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    res = np.concatenate(outs)
    assert res.dtype == frames.dtype and res.shape == frames.shape
    return res


def _render(items, size, fields="first", n_out=None, **kw):
    import pythoncrt_amd as pc
    got, progress = [], []
    n_out = len(items) * (2 if fields == "both" else 1) if n_out is None else n_out
    kw.setdefault("batch", BATCH[fields])
    wrote = pc.process_frames(iter(items), lambda a: got.append(np.array(a)), size[1], size[0], 30.0, n_out, noise_seed=SEED,
                              deinterlace_fields=fields, progress_cb=progress.append, **kw)
    assert wrote == n_out == len(got) and all(a.dtype == np.uint8 for a in got)
    assert progress == [(i + 1) / n_out for i in range(n_out)]                  # frames WRITTEN
    return got


def _check(got, exp, what):
    bad = [(i, int((np.asarray(g).reshape(-1) != np.asarray(e).reshape(-1)).sum())) for i, (g, e) in enumerate(zip(got, exp))
           if np.asarray(g).size != np.asarray(e).size or not np.array_equal(np.asarray(g).reshape(-1), np.asarray(e).reshape(-1))]
    assert len(got) == len(exp) and not bad, (what, bad)
    assert not np.array_equal(got[0], got[1])                                  # frames of a render, not one constant


@pytest.mark.parametrize("method,order,fields", [("linear", "tff", "first"), ("edge", "bff", "both"), ("edge", "tff", "first"), ("linear", "bff", "both")])
def test_rgb24_at_render_size(method, order, fields):
    """pipe(deint(frames)): an rgb24 frame at render size goes through a source end whose only stage is the Deinterlace.  Under "both" the
    writer gets 2 N frames, the chain's frame index runs over them and the persistence state is threaded from one batch of 4 to the next."""
    src = _frames("rgb24", SIZE)
    got = _render(src, SIZE, fields, deinterlace=method, field_order=order)
    assert all(a.shape == SIZE + (3,) for a in got)
    exp = _pipe(model.deinterlace(np.stack(src), method, order, fields), SIZE, BATCH[fields])
    _check(got, exp, ("rgb24", method, order, fields))
    if fields == "both":
        odd = _render(src, SIZE, fields, deinterlace=method, field_order=order, batch=5)       # an odd batch is taken as the even one below it
        _check(odd, exp, "batch=5")
        one = _render(src, SIZE, fields, deinterlace=method, field_order=order, batch=1)       # ... and at least 2
        _check(one, _pipe(model.deinterlace(np.stack(src), method, order, fields), SIZE, 2), "batch=1")
        assert not np.array_equal(np.stack(got)[0::2], np.stack(_render(src, SIZE, "first", deinterlace=method, field_order=order)))   # field rate is another render


def test_uyvy422_and_off_size_nv12():
    """uyvy422 at render size; nv12 at another size: unpacked, deinterlaced AT THE SOURCE SIZE, then resized."""
    h, w = SIZE
    src = _frames("uyvy422", SIZE)
    got = _render(src, SIZE, "both", deinterlace="edge", field_order="bff", in_pix_fmt="uyvy422")
    rgb = np.stack([yuv422_model.unpack(p, h, w, "uyvy422") for p in src])
    _check(got, _pipe(model.deinterlace(rgb, "edge", "bff", "both"), SIZE, 4), "uyvy422")
    sh, sw = 31, 90
    src = _frames("nv12", (sh, sw))
    for fields in model.FIELDS:
        got = _render(src, SIZE, fields, deinterlace="edge", in_pix_fmt="nv12", in_size=(sh, sw))
        rgb = model.deinterlace(np.stack([unpack_model.unpack(p, sh, sw, "nv12") for p in src]), "edge", "tff", fields)
        rgb = np.stack([pil_resize_model.resize(f, h, w) for f in rgb])
        _check(got, _pipe(rgb, SIZE, BATCH[fields]), ("nv12", fields))


def test_ten_bit_source_is_deinterlaced_on_half_frames():
    h, w = SIZE
    src = _frames("p010le", SIZE)
    got = _render(src, SIZE, "both", deinterlace="edge", in_pix_fmt="p010le", out_pix_fmt="yuv420p10le")
    rgb = np.stack([deep_model.unpack(p, h, w, "p010le") for p in src])
    assert rgb.dtype == np.float16
    _check(got, [deep_model.pack(f, "yuv420p10le") for f in _pipe(model.deinterlace(rgb, "edge", "tff", "both"), SIZE, 4)], "p010le")


def test_in_crop_at_an_odd_row_comes_behind_the_deinterlace():
    """rgb24 frames of 30 x 140 with a window of the render size at (3, 2): the fields are separated on the whole source frame, then the
    window is cut — a window cut first would start on the other field."""
    h, w = SIZE
    src = _frames("rgb24", (30, 140), seed=4)
    crop = (3, 2, h, w)
    for method, fields in (("linear", "first"), ("edge", "both")):
        got = _render(src, SIZE, fields, deinterlace=method, field_order="bff", in_crop=crop)
        full = model.deinterlace(np.stack(src), method, "bff", fields)
        _check(got, _pipe(np.ascontiguousarray(full[:, 3:3 + h, 2:2 + w]), SIZE, BATCH[fields]), ("in_crop", method, fields))
        wrong = model.deinterlace(np.stack(src)[:, 3:3 + h, 2:2 + w], method, "bff", fields)
        assert not np.array_equal(wrong, full[:, 3:3 + h, 2:2 + w])


def test_under_a_half_chain_the_deinterlace_runs_on_the_uint8_frames():
    src = _frames("rgb24", SIZE)
    got = _render(src, SIZE, "both", deinterlace="linear", chain_pix="half")
    half = _pipe(depth_model.widen(model.deinterlace(np.stack(src), "linear", "tff", "both")), SIZE, 4)
    _check(got, depth_model.narrow(half, "none"), "chain_pix=half")


def test_mixed_rgb24_source_sizes_and_a_frame_too_small():
    """Frames of two sizes: each is deinterlaced at ITS size and then resized; a batch ends where the size changes, and the stage keeps
    nothing from one frame to the next."""
    import pythoncrt_amd as pc
    h, w = SIZE
    a, b = _frames("rgb24", SIZE, seed=1), _frames("rgb24", (31, 90), seed=2)
    src = [a[0], a[1], b[0], a[2], b[1], b[2], a[3]]
    for fields in model.FIELDS:
        got = _render(src, SIZE, fields, deinterlace="edge", field_order="bff")
        exp = []
        for f in src:
            for g in model.deinterlace(f[None], "edge", "bff", fields):
                exp.append(g if g.shape[:2] == SIZE else pil_resize_model.resize(g, h, w))
        per = 2 if fields == "both" else 1
        # the render loop's batches: at most BATCH[fields] // per source frames of one size
        exp, outs, state, index = np.stack(exp), [], None, 0
        import torch
        from pythoncrt_amd.pipeline import FramePipeline, RenderSettings
        pipe = FramePipeline(_dev(), h, w, RenderSettings(), fps=30.0, noise_seed=SEED, dtype=torch.uint8)
        i = 0
        while i < len(src):
            k = 1
            while k < BATCH[fields] // per and i + k < len(src) and src[i + k].shape == src[i].shape:
                k += 1
            x = torch.from_numpy(exp[i * per:(i + k) * per]).to(_dev())
            out, state = pipe.run(x, first_index=index, state=state)
            torch.cuda.synchronize()
            outs.append(out.cpu().numpy())
            index += k * per
            i += k
        _check(got, np.concatenate(outs), ("mixed", fields))
    with pytest.raises(ValueError, match="no two fields"):
        pc.process_frames(iter([np.zeros((1, w, 3), np.uint8)]), lambda f: None, w, h, 30.0, 1, deinterlace="linear")


@pytest.fixture
def deint_plans(monkeypatch):
    """Records the Deinterlace plans created."""
    from pythoncrt_amd import deint
    made = []
    init0 = deint.Deinterlace.__init__

    def init(self, *a, **kw):
        made.append((a[1:], kw))
        init0(self, *a, **kw)
    monkeypatch.setattr(deint.Deinterlace, "__init__", init)
    return made


def test_off_builds_no_deinterlace(deint_plans):
    import torch
    src = _frames("rgb24", SIZE)
    _check(_render(src, SIZE, batch=2, deinterlace="off", field_order="tff"), _render(src, SIZE, batch=2), "off")
    _check(_render(src, SIZE, batch=2), _pipe(np.stack(src), SIZE, 2), "the chain as it was")
    nv = _frames("nv12", (31, 90))
    _render(nv, SIZE, batch=2, in_pix_fmt="nv12", in_size=(31, 90), in_crop=(1, 0, 24, 80), chain_pix="half")
    assert deint_plans == []
    _render(src, SIZE, "both", deinterlace="edge")
    assert deint_plans == [((SIZE,), {"method": "edge", "order": "tff", "fields": "both", "dtype": torch.uint8})]


@pytest.mark.parametrize("io", ["staged", "mapped"])
@pytest.mark.parametrize("case", [("uyvy422", "rgb24", "edge", "bff", "both", 4), ("rgb24", "nv12", "linear", "tff", "both", 5),
                                  ("p010le", "yuv420p10le", "edge", "tff", "first", 2)], ids=lambda c: "-".join(map(str, c)))
def test_cli_writes_what_process_frames_hands_its_writer(tmp_path, case, io):
    from pythoncrt_amd import cli
    in_fmt, out_fmt, method, order, fields, batch = case
    h, w = SIZE
    per = 2 if fields == "both" else 1
    items = _frames(in_fmt, SIZE)
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    src.write_bytes(b"".join(a.tobytes() for a in items))
    assert cli.main(["--input", str(src), "--output", str(dst), "--width", str(w), "--height", str(h), "--fps", "30", "--batch", str(batch),
                     "--noise-seed", str(SEED), "--in-pix-fmt", in_fmt, "--out-pix-fmt", out_fmt, "--deinterlace", method, "--field-order", order,
                     "--deinterlace-fields", fields, "--io", io]) == 0
    got = _render(items, SIZE, fields, deinterlace=method, field_order=order, in_pix_fmt=in_fmt, out_pix_fmt=out_fmt, batch=batch)
    fb = formats.frame_bytes(h, w, out_fmt)
    written = np.frombuffer(dst.read_bytes(), dtype=np.uint8)
    assert written.size == N * per * fb, (written.size, N, per, fb)            # a file of 2 N delivery frames under "both"
    _check([written[i * fb:(i + 1) * fb] for i in range(N * per)], got, (case, io))
