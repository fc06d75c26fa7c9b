"""process_frames(out_chroma_rows="interlaced") and the CLI on the GPU: what the writer gets is the models' bytes — the source model, the
deinterlace model, [widen], a FramePipeline run by the test itself, [the delivery resize], the weave, [narrow], then the field-paired
egress model (tests/egress_field420_model.py) — composed in the order pythoncrt_amd/ends.py states.  A scene whose two fields are two
flat colours leaves the delivery end with chroma rows that alternate between the two colours with the keyword, and as one mixed colour
without it.  Exact: there is no tolerance."""
import numpy as np
import pytest

from pythoncrt_amd import formats
from tests import deep_model, deint_model, depth_model, field420_model, resize16_model, yuv_model
from tests import egress_field420_model as model
from tests.test_interlace_pipeline_gpu import N, SEED, SIZE, _check, _dev, _frames, _pipe, _render, _weave

pytestmark = pytest.mark.gpu


@pytest.fixture
def made(monkeypatch):
    """Every EgressField420 built: (size, keywords)."""
    from pythoncrt_amd import field420
    log = []
    init0 = field420.EgressField420.__init__

    def init(self, *a, **kw):
        log.append((a[1], kw))
        init0(self, *a, **kw)
    monkeypatch.setattr(field420.EgressField420, "__init__", init)
    return log


def _packed(frames, fmt, chroma="center", matrix="bt601", rng="tv"):
    return [model.pack(f, fmt, chroma, matrix, rng) for f in frames]


# ---- the four configurations ----------------------------------------------------------------------------------------------------------------------

def test_rgb24_field_rate_chain_woven_into_yuv420p(made):
    """rgb24, deinterlace="edge" to both fields, deliver_interlace="tff": N frames in, 2 N through the chain in batches of 4, N woven frames
    out as yuv420p whose chroma rows are formed per field."""
    src = _frames("rgb24", SIZE)
    outs = _pipe(deint_model.deinterlace(np.stack(src), "edge", "tff", "both"), SIZE, 4)
    woven = _weave(outs, "tff", "none")
    got = _render(src, SIZE, N, batch=4, deinterlace="edge", deinterlace_fields="both", deliver_interlace="tff", out_pix_fmt="yuv420p",
                  out_chroma_rows="interlaced")
    _check(got, _packed(woven, "yuv420p"), "rgb24 -> yuv420p, edge both tff")
    assert made == [(SIZE, {"layout": "yuv420p", "matrix": "bt601", "range": "tv", "chroma": "center"})]
    assert not np.array_equal(np.stack(got), np.stack([yuv_model.pack(f, "yuv420p") for f in woven]))       # the progressive plan's bytes are others


def test_nv12_round_trip_with_both_keywords_and_left(made):
    """An interlaced nv12 source read by field, both fields through the chain, woven, and written by field at MPEG-2's siting."""
    h, w = SIZE
    src = _frames("nv12", SIZE, seed=1)
    rgb = field420_model.unpack_batch(src, h, w, "nv12", "replicate")
    outs = _pipe(deint_model.deinterlace(rgb, "linear", "tff", "both"), SIZE, 4)
    got = _render(src, SIZE, N, batch=4, in_pix_fmt="nv12", out_pix_fmt="nv12", in_chroma_rows="interlaced", deinterlace="linear", deinterlace_fields="both",
                  deliver_interlace="tff", out_chroma="left", out_chroma_rows="interlaced", out_matrix="bt709", out_range="pc")
    _check(got, _packed(_weave(outs, "tff", "none"), "nv12", "left", "bt709", "pc"), "nv12 round trip, left")
    assert made == [(SIZE, {"layout": "nv12", "matrix": "bt709", "range": "pc", "chroma": "left"})]


def test_p010le_to_yuv420p10le_passed_through_undeinterlaced(made):
    """No deliver_interlace: a woven source that runs through the chain as it is leaves interlaced too."""
    h, w = SIZE
    src = _frames("p010le", SIZE)
    rgb = np.stack([deep_model.unpack(p, h, w, "p010le") for p in src])
    outs = np.concatenate(_pipe(rgb, SIZE, 2))
    assert outs.dtype == np.float16
    got = _render(src, SIZE, N, batch=2, in_pix_fmt="p010le", out_pix_fmt="yuv420p10le", out_chroma_rows="interlaced")
    _check(got, _packed(outs, "yuv420p10le"), "p010le -> yuv420p10le")
    assert made == [(SIZE, {"layout": "yuv420p10le", "matrix": "bt601", "range": "tv", "chroma": "center"})]


def test_half_chain_with_a_dithered_nv12_delivery_at_another_size(made):
    """chain_pix="half", dither="ordered", deliver_size (36 rows: a multiple of 4), deliver_interlace: resize on halves, the weave at the
    delivery size, the Narrow, then the egress plan built for the delivery size."""
    deliver = (36, 96)
    src = _frames("rgb24", SIZE, seed=2)
    fields = deint_model.deinterlace(np.stack(src), "linear", "bff", "both")
    outs = _pipe(depth_model.widen(fields), SIZE, 4)
    exp = depth_model.narrow(_weave(outs, "bff", "none", lambda f: resize16_model.resize(f, *deliver)), "ordered")
    got = _render(src, SIZE, N, batch=4, deinterlace="linear", field_order="bff", deinterlace_fields="both", chain_pix="half", dither="ordered",
                  deliver_size=deliver, deliver_interlace="bff", out_pix_fmt="nv12", out_chroma="left", out_chroma_rows="interlaced")
    assert all(a.shape == (formats.frame_bytes(36, 96, "nv12"),) for a in got)
    _check(got, _packed(exp, "nv12", "left"), "half, ordered, 36 x 96, nv12 left")
    assert made == [(deliver, {"layout": "nv12", "matrix": "bt601", "range": "tv", "chroma": "left"})]


# ---- two colours, one per field -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,chroma", [("nv12", "center"), ("yuv420p", "left"), ("p010le", "left")])
def test_two_flat_fields_leave_with_chroma_rows_that_alternate(fmt, chroma):
    """The top field is one flat colour and the bottom field another, packed as an interlaced encoder packs them.  Through a SourceEnd
    and a DeliveryEnd with both chroma_rows keywords every chroma plane leaves with exactly two values, one on the rows of each field —
    and the frame is the box stages' for each field's colour; with a progressive delivery end every chroma sample mixes the two."""
    import torch
    from pythoncrt_amd import ends
    size, n = (16, 24), 2
    deep = formats.bits(fmt) == 10
    scale = 4 if deep else 1
    a, b = (60 * scale, 90 * scale, 200 * scale), (180 * scale, 190 * scale, 70 * scale)
    frame = field420_model.two_colour_frame(size[0], size[1], fmt, a, b)
    src = torch.from_numpy(np.stack([frame] * n)).to(_dev())
    pix = torch.float16 if deep else torch.uint8
    source = ends.SourceEnd(_dev(), size, fmt, "bt601", "tv", "replicate", size, "bilinear", None, pix, chroma_rows="interlaced")
    source.slots(n, 1, pinned=False)
    source.dev[0].copy_(src)
    rgb = torch.empty((n,) + size + (3,), dtype=pix, device=_dev())
    source.convert(0, n, rgb)
    outs = {}
    for rows in ("interlaced", "progressive"):
        end = ends.DeliveryEnd(_dev(), size, pix, fmt, "bt601", "tv", chroma, None, "bilinear", chroma_rows=rows)
        end.slots([rgb])
        out = end.run(0, n)
        torch.cuda.synchronize()
        outs[rows] = out.cpu().numpy()
    frames = rgb.cpu().numpy()
    for i in range(n):
        _, u, v = model.samples(outs["interlaced"][i], size[0], size[1], fmt)
        for plane in (u, v):
            assert len(np.unique(plane[0::2])) == 1 and len(np.unique(plane[1::2])) == 1 and plane[0, 0] != plane[1, 0], (fmt, chroma, i)
        assert np.array_equal(outs["interlaced"][i], model.pack(frames[i], fmt, chroma))
        for f in (0, 1):                                            # ... and they are the box stage's samples of a flat frame of the field's colour
            flat = np.ascontiguousarray(np.broadcast_to(frames[i][f, 0], size + (3,)))
            _, fu, fv = model.samples(model.box(flat, fmt), size[0], size[1], fmt)
            assert np.array_equal(u[f::2], fu[f::2]) and np.array_equal(v[f::2], fv[f::2]), (fmt, chroma, i, f)
        _, pu, pv = model.samples(outs["progressive"][i], size[0], size[1], fmt)
        for plane, own in ((pu, u), (pv, v)):
            assert np.array_equal(plane[0::2], plane[1::2])        # no alternation: every row pair mixes the two fields alike
            assert not np.isin(plane, [own[0, 0], own[1, 0]]).any(), (fmt, chroma, i)


# ---- the default, and the CLI -------------------------------------------------------------------------------------------------------------------

def test_progressive_is_the_path_as_it_was(made):
    src = _frames("rgb24", SIZE, seed=3)
    kw = dict(batch=4, deinterlace="linear", deinterlace_fields="both", deliver_interlace="tff", out_pix_fmt="nv12")
    ref = _render(src, SIZE, N, **kw)
    _check(_render(src, SIZE, N, out_chroma_rows="progressive", **kw), ref, "progressive")
    assert made == []
    woven = _weave(_pipe(deint_model.deinterlace(np.stack(src), "linear", "tff", "both"), SIZE, 4), "tff", "none")
    _check(ref, [yuv_model.pack(f, "nv12") for f in woven], "the box plan's bytes")


@pytest.mark.parametrize("io", ["staged", "mapped"])
@pytest.mark.parametrize("case", [("nv12", "nv12", "left", 4), ("p010le", "yuv420p10le", "center", 2)], ids=lambda c: "-".join(map(str, c)))
def test_cli_writes_what_process_frames_hands_its_writer(tmp_path, case, io, made):
    from pythoncrt_amd import cli
    in_fmt, out_fmt, chroma, batch = case
    h, w = SIZE
    items = _frames(in_fmt, SIZE, seed=4)
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    src.write_bytes(b"".join(a.tobytes() for a in items))
    assert cli.main(["--input", str(src), "--output", str(dst), "--width", str(w), "--height", str(h), "--fps", "30", "--batch", str(batch),
                     "--noise-seed", str(SEED), "--in-pix-fmt", in_fmt, "--out-pix-fmt", out_fmt, "--out-chroma", chroma, "--out-chroma-rows", "interlaced",
                     "--in-chroma-rows", "interlaced", "--deinterlace", "linear", "--deinterlace-fields", "both", "--deliver-interlace", "tff", "--io", io]) == 0
    assert [m[1]["chroma"] for m in made] == [chroma] and made[0][0] == SIZE
    got = _render(items, SIZE, N, in_chroma_rows="interlaced", out_chroma_rows="interlaced", out_chroma=chroma, deinterlace="linear", deinterlace_fields="both",
                  deliver_interlace="tff", in_pix_fmt=in_fmt, out_pix_fmt=out_fmt, batch=batch)
    fb = formats.frame_bytes(h, w, out_fmt)
    written = np.frombuffer(dst.read_bytes(), dtype=np.uint8)
    assert written.size == N * fb, (written.size, N, fb)
    _check([written[i * fb:(i + 1) * fb] for i in range(N)], got, (case, io))
    # ... and they are the models' bytes
    rgb = deint_model.deinterlace(field420_model.unpack_batch(items, h, w, in_fmt, "replicate"), "linear", "tff", "both")
    _check(got, _packed(_weave(_pipe(rgb, SIZE, batch), "tff", "none"), out_fmt, chroma), (case, "models"))
