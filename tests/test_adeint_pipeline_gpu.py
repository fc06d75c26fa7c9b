"""process_frames(deinterlace="adaptive") and the CLI's --deinterlace adaptive on the GPU: what the writer gets is the models' bytes — the
source model, tests/adeint_model at the SOURCE size over the WHOLE sequence (the history crosses the render loop's batches), the resize
model, [widen], a FramePipeline run by the test itself, [narrow], the egress model — composed in the order pythoncrt_amd/ends.py states.
5 source frames whose successors keep part of the picture; under "first" in batches of 2, under "both" 10 frames in chain batches of 4.
Exact: there is no tolerance."""
import numpy as np
import pytest

from pythoncrt_amd import formats
from tests import adeint_model as model
from tests import deep_model, deint_model, depth_model, pil_resize_model, unpack_model, yuv422_model

pytestmark = pytest.mark.gpu

N, SEED = 5, 29
SIZE = (24, 136)
BATCH = {"first": 2, "both": 4}         # the chain's batch: under "both" two source frames feed it
ALL = {"weave", "held", "edge"}


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _frames(fmt, size, seed=0, n=N):
    """n frames of `fmt` as process_frames takes them (H x W x 3 for rgb24, else 1-D uint8 of frame_bytes; 10-bit samples are valid ones),
    each the one before it with runs of 16 samples redrawn — wholly, or by a few codes — so that part of the picture stands still."""
    h, w = size
    rng = np.random.default_rng([h, w, seed, sum(map(ord, fmt))])
    deep = fmt != "rgb24" and formats.bits(fmt) == 10
    count = h * w * 3 if fmt == "rgb24" else formats.frame_bytes(h, w, fmt) // (2 if deep else 1)
    top = 1024 if deep else 256
    out, cur = [], rng.integers(0, top, count)
    for _ in range(n):
        u = np.repeat(rng.random((count + 15) // 16), 16)[:count]
        cur = np.where(u < 0.25, rng.integers(0, top, count), np.where(u < 0.45, np.clip(cur + rng.integers(-6, 7, count), 0, top - 1), cur))
        if fmt == "rgb24":
            out.append(cur.astype(np.uint8).reshape(h, w, 3))
        elif not deep:
            out.append(cur.astype(np.uint8))
        else:
            out.append((cur.astype(np.uint16) << (6 if fmt == "p010le" else 0)).astype("<u2").view(np.uint8))
    return out


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
    return np.concatenate(outs)


def _render(items, size, fields="first", n_out=None, **kw):
    import pythoncrt_amd as pc
    got = []
    n_out = len(items) * (2 if fields == "both" else 1) if n_out is None else n_out
    kw.setdefault("batch", BATCH[fields])
    wrote = pc.process_frames(iter(items), lambda a: got.append(np.array(a)), size[1], size[0], 30.0, n_out, noise_seed=SEED,
                              deinterlace_fields=fields, **kw)
    assert wrote == n_out == len(got) and all(a.dtype == np.uint8 for a in got)
    return got


def _check(got, exp, what):
    bad = [(i, int((np.asarray(g).reshape(-1) != np.asarray(e).reshape(-1)).sum())) for i, (g, e) in enumerate(zip(got, exp))
           if np.asarray(g).size != np.asarray(e).size or not np.array_equal(np.asarray(g).reshape(-1), np.asarray(e).reshape(-1))]
    assert len(got) == len(exp) and not bad, (what, bad)
    assert not np.array_equal(got[0], got[1])                                  # frames of a render, not one constant


def _adaptive(rgb, order, fields):
    """The model over the whole sequence — and the sequence is one that tells the methods apart: every clamp class occurs behind frame 0."""
    out, parts = model.adaptive_parts(rgb, None, order, fields)
    assert model.clamp_classes(parts) == ALL
    assert not np.array_equal(deint_model.bits(out), deint_model.bits(deint_model.deinterlace(rgb, "edge", order, fields)))
    return out


@pytest.mark.parametrize("order,fields", [("tff", "first"), ("bff", "both")])
def test_rgb24_at_render_size(order, fields):
    src = _frames("rgb24", SIZE)
    got = _render(src, SIZE, fields, deinterlace="adaptive", field_order=order)
    exp = _pipe(_adaptive(np.stack(src), order, fields), SIZE, BATCH[fields])
    _check(got, exp, ("rgb24", order, fields))
    # the history crosses the batches: per-batch histories would be another render
    per = 2 if fields == "both" else 1
    cut = np.concatenate([model.adaptive(np.stack(src[lo:lo + BATCH[fields] // per]), None, order, fields) for lo in range(0, N, BATCH[fields] // per)])
    assert not np.array_equal(cut, model.adaptive(np.stack(src), None, order, fields))
    one = _render(src, SIZE, fields, deinterlace="adaptive", field_order=order, batch=1)       # one source frame per batch
    _check(one, _pipe(model.adaptive(np.stack(src), None, order, fields), SIZE, per), "batch=1")


@pytest.mark.parametrize("fields", model.FIELDS)
def test_uyvy422_and_off_size_nv12(fields):
    """uyvy422 at render size; nv12 at another size: unpacked, deinterlaced AT THE SOURCE SIZE over the whole sequence, then resized."""
    h, w = SIZE
    src = _frames("uyvy422", SIZE)
    got = _render(src, SIZE, fields, deinterlace="adaptive", field_order="bff", in_pix_fmt="uyvy422")
    rgb = np.stack([yuv422_model.unpack(p, h, w, "uyvy422") for p in src])
    _check(got, _pipe(_adaptive(rgb, "bff", fields), SIZE, BATCH[fields]), "uyvy422")
    sh, sw = 31, 90
    src = _frames("nv12", (sh, sw))
    got = _render(src, SIZE, fields, deinterlace="adaptive", in_pix_fmt="nv12", in_size=(sh, sw))
    rgb = _adaptive(np.stack([unpack_model.unpack(p, sh, sw, "nv12") for p in src]), "tff", fields)
    rgb = np.stack([pil_resize_model.resize(f, h, w) for f in rgb])
    _check(got, _pipe(rgb, SIZE, BATCH[fields]), ("nv12", fields))


@pytest.mark.parametrize("fields", model.FIELDS)
def test_ten_bit_source_and_a_half_chain(fields):
    h, w = SIZE
    src = _frames("p010le", SIZE)
    got = _render(src, SIZE, fields, deinterlace="adaptive", in_pix_fmt="p010le", out_pix_fmt="yuv420p10le")
    rgb = np.stack([deep_model.unpack(p, h, w, "p010le") for p in src])
    assert rgb.dtype == np.float16
    _check(got, [deep_model.pack(f, "yuv420p10le") for f in _pipe(_adaptive(rgb, "tff", fields), SIZE, BATCH[fields])], "p010le")
    src = _frames("rgb24", SIZE, seed=3)                                        # chain_pix="half": the stage runs on the uint8 frames in front of the Widen
    got = _render(src, SIZE, fields, deinterlace="adaptive", chain_pix="half")
    half = _pipe(depth_model.widen(_adaptive(np.stack(src), "tff", fields)), SIZE, BATCH[fields])
    _check(got, depth_model.narrow(half, "none"), "chain_pix=half")


@pytest.mark.parametrize("fields", model.FIELDS)
def test_mixed_rgb24_source_sizes_start_a_new_history(fields):
    """Frames of two sizes: a batch ends where the size changes and the first frame behind every change is EDGE's, though a frame of its
    size was converted earlier; within a run of one size the history crosses the batches."""
    import torch
    from pythoncrt_amd.pipeline import FramePipeline, RenderSettings
    h, w = SIZE
    a, b = _frames("rgb24", SIZE, seed=1, n=6), _frames("rgb24", (31, 90), seed=2, n=3)
    src = [a[0], a[1], a[2], b[0], a[3], b[1], b[2], a[4], a[5]]
    per = 2 if fields == "both" else 1
    runs, i = [], 0
    while i < len(src):
        k = 1
        while i + k < len(src) and src[i + k].shape == src[i].shape:
            k += 1
        runs.append((i, k))
        i += k
    assert [k for _, k in runs] == [3, 1, 1, 2, 2]
    exp = []
    for i, k in runs:
        run = model.adaptive(np.stack(src[i:i + k]), None, "bff", fields)
        assert np.array_equal(run[:per], deint_model.deinterlace(src[i][None], "edge", "bff", fields))     # the first frame behind a change: EDGE's
        for g in run:
            exp.append(g if g.shape[:2] == SIZE else pil_resize_model.resize(g, h, w))
    # a[3] behind b[0]: with a[2] as its previous frame it would be another frame
    assert not np.array_equal(model.adaptive(a[3][None], a[2], "bff", fields), model.adaptive(a[3][None], None, "bff", fields))
    got = _render(src, SIZE, fields, deinterlace="adaptive", field_order="bff")
    exp, outs, state, index = np.stack(exp), [], None, 0
    pipe = FramePipeline(_dev(), h, w, RenderSettings(), fps=30.0, noise_seed=SEED, dtype=torch.uint8)
    for i, k in runs:                                                           # the render loop's batches: at most BATCH // per source frames of one size
        for lo in range(i, i + k, BATCH[fields] // per):
            n = min(BATCH[fields] // per, i + k - lo)
            out, state = pipe.run(torch.from_numpy(exp[lo * per:(lo + n) * per]).to(_dev()), first_index=index, state=state)
            torch.cuda.synchronize()
            outs.append(out.cpu().numpy())
            index += n * per
    _check(got, np.concatenate(outs), ("mixed", fields))


def test_edge_and_off_build_no_adaptive_plan(monkeypatch):
    from pythoncrt_amd import adeint
    made = []
    init0 = adeint.AdaptiveDeinterlace.__init__

    def init(self, *a, **kw):
        made.append((a[1:], kw))
        init0(self, *a, **kw)
    monkeypatch.setattr(adeint.AdaptiveDeinterlace, "__init__", init)
    import torch
    src = _frames("rgb24", SIZE)
    _check(_render(src, SIZE, batch=2, deinterlace="off"), _pipe(np.stack(src), SIZE, 2), "off")
    for method, fields in (("edge", "both"), ("linear", "first")):
        got = _render(src, SIZE, fields, deinterlace=method)
        _check(got, _pipe(deint_model.deinterlace(np.stack(src), method, "tff", fields), SIZE, BATCH[fields]), method)
    assert made == []
    _render(src, SIZE, "both", deinterlace="adaptive")
    assert made == [((SIZE,), {"order": "tff", "fields": "both", "dtype": torch.uint8})]


@pytest.mark.parametrize("io", ["staged", "mapped"])
@pytest.mark.parametrize("case", [("uyvy422", "rgb24", "bff", "both", 4), ("rgb24", "nv12", "tff", "first", 2)], ids=lambda c: "-".join(map(str, c)))
def test_cli_writes_what_process_frames_hands_its_writer(tmp_path, case, io):
    from pythoncrt_amd import cli
    in_fmt, out_fmt, order, fields, batch = case
    h, w = SIZE
    per = 2 if fields == "both" else 1
    items = _frames(in_fmt, SIZE)
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    src.write_bytes(b"".join(a.tobytes() for a in items))
    assert cli.main(["--input", str(src), "--output", str(dst), "--width", str(w), "--height", str(h), "--fps", "30", "--batch", str(batch),
                     "--noise-seed", str(SEED), "--in-pix-fmt", in_fmt, "--out-pix-fmt", out_fmt, "--deinterlace", "adaptive", "--field-order", order,
                     "--deinterlace-fields", fields, "--io", io]) == 0
    got = _render(items, SIZE, fields, deinterlace="adaptive", field_order=order, in_pix_fmt=in_fmt, out_pix_fmt=out_fmt, batch=batch)
    fb = formats.frame_bytes(h, w, out_fmt)
    written = np.frombuffer(dst.read_bytes(), dtype=np.uint8)
    assert written.size == N * per * fb, (written.size, N, per, fb)
    _check([written[i * fb:(i + 1) * fb] for i in range(N * per)], got, (case, io))
