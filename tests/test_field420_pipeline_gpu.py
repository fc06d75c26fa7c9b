"""process_frames(in_chroma_rows="interlaced"), probe_frames and the CLI on the GPU: what the writer gets is the models' bytes — the
field-paired source model (tests/field420_model.py), the deinterlace model at the SOURCE size, the resize model, [widen], a FramePipeline
run by the test itself, [narrow], the egress model — composed in the order pythoncrt_amd/ends.py states.  A scene whose two fields are two
flat colours leaves the source end as flat frames with the keyword and as striped ones without it.  Exact: there is no tolerance."""
import numpy as np
import pytest

from pythoncrt_amd import formats, probe
from tests import adeint_model, deep_model, deint_model, depth_model, pil_resize_model, probe_model, unpack_model
from tests import field420_model as model
from tests.test_adeint_pipeline_gpu import SEED, _check, _dev, _frames, _pipe

pytestmark = pytest.mark.gpu

N = 5
SIZE = (24, 136)


def _render(items, size, n_out, **kw):
    import pythoncrt_amd as pc
    got = []
    wrote = pc.process_frames(iter(items), lambda a: got.append(np.array(a)), size[1], size[0], 30.0, n_out, noise_seed=SEED, **kw)
    assert wrote == n_out == len(got) and all(a.dtype == np.uint8 for a in got)
    return got


@pytest.fixture
def made(monkeypatch):
    """Every UnpackField420 built: (size, keywords)."""
    from pythoncrt_amd import field420
    log = []
    init0 = field420.UnpackField420.__init__

    def init(self, *a, **kw):
        log.append((a[1], kw))
        init0(self, *a, **kw)
    monkeypatch.setattr(field420.UnpackField420, "__init__", init)
    return log


def _rgb(src, size, fmt, chroma="replicate"):
    return model.unpack_batch(src, size[0], size[1], fmt, chroma)


# ---- the four configurations ----------------------------------------------------------------------------------------------------------------------

def test_yuv420p_linear_both_fields(made):
    src = _frames("yuv420p", SIZE)
    got = _render(src, SIZE, 2 * N, batch=4, in_pix_fmt="yuv420p", in_chroma_rows="interlaced", deinterlace="linear", deinterlace_fields="both")
    rgb = _rgb(src, SIZE, "yuv420p")
    assert not np.array_equal(rgb, np.stack([unpack_model.unpack(p, SIZE[0], SIZE[1], "yuv420p") for p in src]))
    _check(got, _pipe(deint_model.deinterlace(rgb, "linear", "tff", "both"), SIZE, 4), "yuv420p linear both")
    assert made == [(SIZE, {"layout": "yuv420p", "matrix": "bt601", "range": "tv", "chroma": "replicate"})]


def test_off_size_nv12_edge(made):
    """nv12 at another size: unpacked by field, deinterlaced AT THE SOURCE SIZE, then resized."""
    sh, sw = 30, 90
    src = _frames("nv12", (sh, sw))
    got = _render(src, SIZE, N, batch=2, in_pix_fmt="nv12", in_size=(sh, sw), in_chroma_rows="interlaced", deinterlace="edge", field_order="bff")
    rgb = deint_model.deinterlace(_rgb(src, (sh, sw), "nv12"), "edge", "bff", "first")
    rgb = np.stack([pil_resize_model.resize(f, SIZE[0], SIZE[1]) for f in rgb])
    _check(got, _pipe(rgb, SIZE, 2), "off-size nv12 edge")
    assert made == [((sh, sw), {"layout": "nv12", "matrix": "bt601", "range": "tv", "chroma": "replicate"})]


def test_p010le_adaptive_in_batches_smaller_than_the_sequence(made):
    src = _frames("p010le", SIZE)
    got = _render(src, SIZE, N, batch=2, in_pix_fmt="p010le", out_pix_fmt="yuv420p10le", in_chroma_rows="interlaced", in_chroma="center",
                  deinterlace="adaptive")
    rgb = _rgb(src, SIZE, "p010le", "center")
    assert rgb.dtype == np.float16
    out = _pipe(adeint_model.adaptive(rgb, None, "tff", "first"), SIZE, 2)
    _check(got, [deep_model.pack(f, "yuv420p10le") for f in out], "p010le adaptive")
    assert made == [(SIZE, {"layout": "p010le", "matrix": "bt601", "range": "tv", "chroma": "center"})]


def test_a_half_chain_with_in_chroma_left(made):
    """chain_pix="half": the source stages run on uint8 frames in front of the Widen."""
    src = _frames("nv12", SIZE, seed=3)
    got = _render(src, SIZE, N, batch=2, in_pix_fmt="nv12", in_chroma_rows="interlaced", in_chroma="left", chain_pix="half", deinterlace="linear",
                  in_matrix="bt709", in_range="pc")
    rgb = model.unpack_batch(src, SIZE[0], SIZE[1], "nv12", "left", "bt709", "pc")
    half = _pipe(depth_model.widen(deint_model.deinterlace(rgb, "linear", "tff", "first")), SIZE, 2)
    _check(got, depth_model.narrow(half, "none"), "chain_pix=half, in_chroma=left")
    assert made == [(SIZE, {"layout": "nv12", "matrix": "bt709", "range": "pc", "chroma": "left"})]


# ---- two colours, one per field -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,chroma", [("nv12", "replicate"), ("yuv420p", "left"), ("p010le", "center")])
def test_two_flat_fields_leave_the_source_end_as_flat_frames(fmt, chroma):
    """The top field is one flat colour and the bottom field another, packed as an interlaced encoder packs them.  Behind the source plan
    and Deinterlace("linear", both fields) every frame is ONE colour with the keyword — the top field's, then the bottom field's — and
    with "progressive" no frame is: rows 4j + 1 and 4j + 2 carry the other field's chroma."""
    import torch
    from pythoncrt_amd import ends
    size, n = (16, 24), 2
    deep = formats.bits(fmt) == 10
    scale = 4 if deep else 1
    a, b = (60 * scale, 90 * scale, 200 * scale), (180 * scale, 190 * scale, 70 * scale)
    frame = model.two_colour_frame(size[0], size[1], fmt, a, b)
    src = torch.from_numpy(np.stack([frame] * n)).to(_dev())
    pix = torch.float16 if deep else torch.uint8
    outs = {}
    for rows in ("interlaced", "progressive"):
        end = ends.SourceEnd(_dev(), size, fmt, "bt601", "tv", chroma, size, "bilinear", None, pix, deinterlace=("linear", "tff", "both"), chroma_rows=rows)
        end.slots(n, 1, pinned=False)
        end.dev[0].copy_(src)
        dst = torch.empty((2 * n,) + size + (3,), dtype=pix, device=_dev())
        end.convert(0, n, dst)
        torch.cuda.synchronize()
        outs[rows] = dst.cpu().numpy()
    flat = [model.unpack(model.pack_planes(*(np.full(s, c) for s, c in zip(((4, 8), (2, 4), (2, 4)), col)), fmt), 4, 8, fmt)[0, 0] for col in (a, b)]
    assert not np.array_equal(flat[0], flat[1])
    for i, f in enumerate(outs["interlaced"]):
        assert (deint_model.bits(f) == deint_model.bits(flat[i % 2])).all(), (fmt, chroma, i)
    for i, f in enumerate(outs["progressive"]):
        assert len(np.unique(deint_model.bits(f).reshape(-1, 3), axis=0)) > 1, (fmt, chroma, i)


# ---- probe_frames ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["nv12", "yuv420p10le"])
def test_probe_frames_reads_the_field_paired_source(fmt):
    """A woven stream of coloured motion: the records are the model's on the RGB of the field-paired source model, in batches smaller than
    the stream; without the keyword they are those of the progressive source."""
    import pythoncrt_amd as pc
    size = (32, 48)
    src = _frames(fmt, size, seed=7, n=6)
    rep = pc.probe_frames(iter(src), size[1], size[0], in_pix_fmt=fmt, batch=4, in_chroma_rows="interlaced", in_chroma="left")
    exp = probe.ProbeReport(size).add(probe_model.records(_rgb(src, size, fmt, "left")))
    old = pc.probe_frames(iter(src), size[1], size[0], in_pix_fmt=fmt, batch=4, in_chroma="left")
    for name in ("frames", "pairs", "s_cur", "s_even", "s_odd", "sum_y", "rgb_min", "rgb_max"):
        assert getattr(rep, name) == getattr(exp, name), name
    for name in ("hist", "row_max", "col_max"):
        assert np.array_equal(getattr(rep, name), getattr(exp, name)), name
    assert rep.frames == 6 and rep.pairs == 5 and (old.s_even, old.s_odd) != (rep.s_even, rep.s_odd)


# ---- the default, and the CLI -------------------------------------------------------------------------------------------------------------------

def test_progressive_is_the_path_as_it_was(made):
    src = _frames("nv12", SIZE)
    ref = _pipe(deint_model.deinterlace(np.stack([unpack_model.unpack(p, SIZE[0], SIZE[1], "nv12") for p in src]), "linear", "tff", "first"), SIZE, 2)
    for extra in ({}, dict(in_chroma_rows="progressive")):
        _check(_render(src, SIZE, N, batch=2, in_pix_fmt="nv12", deinterlace="linear", **extra), ref, extra)
    assert made == []


@pytest.mark.parametrize("io", ["staged", "mapped"])
@pytest.mark.parametrize("case", [("nv12", "rgb24", "left", "both", 4), ("p010le", "yuv420p10le", "replicate", "first", 2)], ids=lambda c: "-".join(map(str, c)))
def test_cli_writes_what_process_frames_hands_its_writer(tmp_path, case, io, made):
    from pythoncrt_amd import cli
    in_fmt, out_fmt, chroma, fields, batch = case
    h, w = SIZE
    per = 2 if fields == "both" else 1
    items = _frames(in_fmt, SIZE)
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    src.write_bytes(b"".join(a.tobytes() for a in items))
    assert cli.main(["--input", str(src), "--output", str(dst), "--width", str(w), "--height", str(h), "--fps", "30", "--batch", str(batch),
                     "--noise-seed", str(SEED), "--in-pix-fmt", in_fmt, "--out-pix-fmt", out_fmt, "--in-chroma", chroma, "--in-chroma-rows", "interlaced",
                     "--deinterlace", "edge", "--deinterlace-fields", fields, "--io", io]) == 0
    assert [m[1]["chroma"] for m in made] == [chroma]
    got = _render(items, SIZE, N * per, in_chroma_rows="interlaced", in_chroma=chroma, deinterlace="edge", deinterlace_fields=fields, in_pix_fmt=in_fmt,
                  out_pix_fmt=out_fmt, batch=batch)
    fb = formats.frame_bytes(h, w, out_fmt)
    written = np.frombuffer(dst.read_bytes(), dtype=np.uint8)
    assert written.size == N * per * fb, (written.size, N, per, fb)
    _check([written[i * fb:(i + 1) * fb] for i in range(N * per)], got, (case, io))
    # ... and they are the models' bytes
    rgb = deint_model.deinterlace(_rgb(items, SIZE, in_fmt, chroma), "edge", "tff", fields)
    out = _pipe(rgb, SIZE, batch)
    _check(got, out if out_fmt == "rgb24" else [deep_model.pack(f, out_fmt) for f in out], (case, "models"))
