"""process_frames(in_lut=, deliver_lut=) and the CLI's --in-lut / --deliver-lut on the GPU: what the writer gets is the models' bytes — the
source model, the resize model, tests/depth_model.widen, tests/lut3d_model.apply, a FramePipeline run by the test itself, lut3d_model.apply
again, the geometry models, depth_model.narrow, the egress model — composed in the order pythoncrt_amd/ends.py states.  5 frames in
batches of 2 (the last one partial), the default persistence carrying state across batches, the grain fixed by noise_seed.  Exact: there
is no tolerance."""
import numpy as np
import pytest

from pythoncrt_amd import formats
from pythoncrt_amd.cube import Cube
from tests import canvas_model, deep444_model, deep_model, depth_model, pil_resize_model, resize16_model, unpack_model, yuv_model
from tests import lut3d_model as model

pytestmark = pytest.mark.gpu

N, BATCH, SEED = 5, 2, 23
SIZE = (23, 131)


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _cube(n, seed):
    t = model.random_table(n, seed)
    c = Cube(n, t.astype(np.float64) / 1020.0)
    assert np.array_equal(c.quantise(), t)
    return c, t


IN_CUBE, IN_TABLE = _cube(17, 41)
OUT_CUBE, OUT_TABLE = _cube(35, 42)             # one cube per table path


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


def _pipe(frames, size):
    """A FramePipeline of the frames' dtype with process_frames' default settings over [N, h, w, 3], in batches of BATCH with the state
    carried as the render loop carries it."""
    import torch
    from pythoncrt_amd.pipeline import FramePipeline, RenderSettings
    h, w = size
    x = torch.from_numpy(np.ascontiguousarray(frames)).to(_dev())
    pipe = FramePipeline(_dev(), h, w, RenderSettings(), fps=30.0, noise_seed=SEED, dtype=x.dtype)
    outs, state = [], None
    for lo in range(0, N, BATCH):
        out, state = pipe.run(x[lo:lo + BATCH], first_index=lo, state=state)
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    res = np.concatenate(outs)
    assert res.dtype == frames.dtype and res.shape == (N, h, w, 3)
    return res


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


def test_in_lut_on_rgb24(tmp_path):
    """pipe(lut(frames)) on the uint8 chain: an rgb24 frame at render size goes through a source end whose only stage is the LUT.  The
    cube comes from a .cube file."""
    path = tmp_path / "in.cube"
    model.write_cube(path, IN_CUBE.values)
    src = _frames("rgb24", SIZE)
    got = _render(src, SIZE, in_lut=str(path))
    assert all(a.shape == SIZE + (3,) for a in got)
    exp = _pipe(model.apply(np.stack(src), IN_TABLE), SIZE)
    _check(got, exp, "rgb24")
    assert not np.array_equal(np.stack(got), np.stack(_render(src, SIZE)))      # the cube does something


def test_in_lut_behind_the_resize_of_an_off_size_nv12_source():
    h, w = SIZE
    sh, sw = 31, 90
    src = _frames("nv12", (sh, sw))
    got = _render(src, SIZE, in_pix_fmt="nv12", in_size=(sh, sw), in_lut=IN_CUBE)
    rgb = np.stack([pil_resize_model.resize(unpack_model.unpack(p, sh, sw, "nv12"), h, w) for p in src])
    _check(got, _pipe(model.apply(rgb, IN_TABLE), SIZE), "nv12")


def test_in_lut_sees_halves_under_a_half_chain():
    """rgb24 -> Widen -> LUT on halves (S = 1020) -> half chain -> Narrow: not the bytes of the LUT on uint8 codes followed by a Widen."""
    src = np.stack(_frames("rgb24", SIZE))
    got = _render(list(src), SIZE, chain_pix="half", in_lut=IN_CUBE)
    wide = model.apply(depth_model.widen(src), IN_TABLE)
    assert wide.dtype == np.float16
    _check(got, depth_model.narrow(_pipe(wide, SIZE), "none"), "half")
    assert not np.array_equal(wide, depth_model.widen(model.apply(src, IN_TABLE)))      # half precision: quarter codes, not uint8 codes


def _delivered(rendered_half, size, deliver, color):
    """lut -> resize -> pad on halves, then the ordered Narrow, then nv12: the delivery of the test below from the models."""
    inner, at = canvas_model.fit_pad(size, deliver)
    assert inner != deliver and inner != size                                  # a resize and a Canvas stand between the LUT and the Narrow
    half = model.apply(rendered_half, OUT_TABLE)
    half = resize16_model.resize(half, *inner)
    half = canvas_model.canvas(half, deliver, at=at, fill=np.array(color, dtype=np.float16))
    return [yuv_model.pack(f, "nv12") for f in depth_model.narrow(half, "ordered")]


def test_deliver_lut_stands_in_front_of_the_delivery_geometry():
    """rgb24 -> nv12 on a half chain with deliver_size, deliver_fit="pad" and the ordered dither: the LUT runs at render size on the
    finished half frames; the pad colour is not transformed and the dither stays last."""
    deliver, color = (36, 96), (7, 200, 33)
    src = np.stack(_frames("rgb24", SIZE))
    got = _render(list(src), SIZE, chain_pix="half", dither="ordered", out_pix_fmt="nv12", deliver_size=deliver, deliver_fit="pad",
                  deliver_pad_color=color, deliver_lut=OUT_CUBE)
    _check(got, _delivered(_pipe(depth_model.widen(src), SIZE), SIZE, deliver, color), "pad")
    bars = yuv_model.pack(np.broadcast_to(np.array(color, dtype=np.uint8), deliver + (3,)).copy(), "nv12")
    assert np.array_equal(got[0][:96 * 2], bars[:96 * 2])                       # the top rows of luma are bar: the pad colour as given


def test_both_keywords_between_two_ten_bit_ends():
    h, w = SIZE
    src = _frames("p010le", SIZE)
    got = _render(src, SIZE, in_pix_fmt="p010le", out_pix_fmt="x2rgb10le", in_lut=IN_CUBE, deliver_lut=OUT_CUBE)
    rgb = np.stack([deep_model.unpack(p, h, w, "p010le") for p in src])
    out = model.apply(_pipe(model.apply(rgb, IN_TABLE), SIZE), OUT_TABLE)
    _check(got, [deep444_model.pack(f, "x2rgb10le") for f in out], "p010le")


def test_two_large_lds_cubes_of_different_sizes_in_one_render():
    """deliver_lut N = 33 (143 748 bytes of LDS) is created first, in_lut N = 32 (131 072) behind it, for the same sample type: the
    second plan's create must not lower the kernel's dynamic-LDS limit under the first."""
    in_cube, in_table = _cube(32, 43)
    out_cube, out_table = _cube(33, 44)
    src = _frames("rgb24", SIZE)
    got = _render(src, SIZE, in_lut=in_cube, deliver_lut=out_cube)
    _check(got, model.apply(_pipe(model.apply(np.stack(src), in_table), SIZE), out_table), "33 behind 32")


@pytest.fixture
def lut_plans(monkeypatch):
    """Counts the Lut3D plans created, by dtype."""
    from pythoncrt_amd import lut3d
    made = []
    init0 = lut3d.Lut3D.__init__

    def init(self, *a, **kw):
        made.append(str(kw.get("dtype")))
        init0(self, *a, **kw)
    monkeypatch.setattr(lut3d.Lut3D, "__init__", init)
    return made


def test_an_identity_cube_and_none(lut_plans):
    """On the uint8 chain an identity cube returns every code unchanged: the bytes of a run without it, on either end and on both; None
    builds no Lut3D."""
    for fmt_kw in (dict(), dict(in_pix_fmt="nv12", out_pix_fmt="yuv420p")):
        src = _frames(fmt_kw.get("in_pix_fmt", "rgb24"), SIZE)
        plain = _render(src, SIZE, in_lut=None, deliver_lut=None, **fmt_kw)
        _check(_render(src, SIZE, **fmt_kw), plain, "defaults")
        assert lut_plans == []
        _check(_render(src, SIZE, in_lut=Cube.identity(33), **fmt_kw), plain, "in")
        _check(_render(src, SIZE, deliver_lut=Cube.identity(2), **fmt_kw), plain, "deliver")
        _check(_render(src, SIZE, in_lut=Cube.identity(65), deliver_lut=Cube.identity(17), **fmt_kw), plain, "both")
        assert lut_plans == ["torch.uint8"] * 4                                 # deliver end first, then the source end
        del lut_plans[:]


@pytest.mark.parametrize("io", ["staged", "mapped"])
def test_cli_writes_what_process_frames_hands_its_writer(tmp_path, io):
    from pythoncrt_amd import cli
    h, w = SIZE
    in_path, out_path = tmp_path / "in.cube", tmp_path / "out.cube"
    model.write_cube(in_path, IN_CUBE.values)
    model.write_cube(out_path, OUT_CUBE.values)
    for in_fmt, out_fmt, extra, kw in (
            ("rgb24", "rgb24", [], {}),
            ("rgb24", "nv12", ["--chain-pix", "half", "--dither", "ordered", "--deliver-height", "36", "--deliver-width", "96", "--deliver-fit", "pad",
                               "--deliver-pad-color", "7,200,33"],
             dict(chain_pix="half", dither="ordered", deliver_size=(36, 96), deliver_fit="pad", deliver_pad_color=(7, 200, 33)))):
        items = _frames(in_fmt, SIZE)
        src, dst = tmp_path / f"in_{out_fmt}.raw", tmp_path / f"out_{out_fmt}.raw"
        src.write_bytes(b"".join(a.tobytes() for a in items))
        assert cli.main(["--input", str(src), "--output", str(dst), "--width", str(w), "--height", str(h), "--fps", "30", "--batch", str(BATCH),
                         "--noise-seed", str(SEED), "--in-pix-fmt", in_fmt, "--out-pix-fmt", out_fmt, "--in-lut", str(in_path),
                         "--deliver-lut", str(out_path), "--io", io] + extra) == 0
        got = _render(items, SIZE, in_pix_fmt=in_fmt, out_pix_fmt=out_fmt, in_lut=str(in_path), deliver_lut=str(out_path), **kw)
        fb = formats.frame_bytes(*((36, 96) if extra else SIZE), out_fmt)
        written = np.frombuffer(dst.read_bytes(), dtype=np.uint8)
        assert written.size == N * fb, (written.size, N, fb)
        _check([written[i * fb:(i + 1) * fb] for i in range(N)], got, (out_fmt, io))
        if not extra:                                                           # ... which are the models' bytes
            exp = model.apply(_pipe(model.apply(np.stack(items), IN_TABLE), SIZE), OUT_TABLE)
            _check(got, exp, "models")
