"""The sited egress stage on the GPU: EgressSited (k_egress_sited, seven layouts x vec / general, siting left / center) against the int64
host model of tests/egress_sited_model.py — equality is zero differing elements, and every assert names the plan string — against the box
stages on the device for the same input ("center" is their bytes, "left" is not), and process_frames / the CLI with out_chroma against the
model of their own rgb24 output."""
import functools

import numpy as np
import pytest

from pythoncrt_amd import _lib
from tests import deep_model
from tests import egress_sited_model as model

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (2, 2), (3, 5), (5, 3), (4, 8), (6, 24), (5, 520), (37, 131)]
LAYOUTS = list(model.LAYOUTS)
SITINGS = list(model.SITINGS)
ids = dict(ids=lambda s: f"{s[0]}x{s[1]}")


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _name(layout, vec, siting, frames):
    return f"egress_sited=k_egress_sited<{layout},{'vec' if vec else 'general'}>;siting={siting};frames={frames}"


def _run(frames_np, layout, siting="left", force_general=False, matrix="bt601", rng="tv"):
    """(uint8 [n, frame_bytes] from the device, last_plan) for a stack of RGB frames."""
    import torch
    from pythoncrt_amd import EgressSited
    size = tuple(frames_np.shape[1:3])
    plan = EgressSited(_dev(), size, layout, matrix=matrix, range=rng, siting=siting, force_general=force_general)
    assert plan.siting == siting and plan.force_general == force_general and plan.frame_bytes == model.frame_bytes(size[0], size[1], layout)
    out = plan(torch.from_numpy(frames_np).to(_dev()))
    torch.cuda.synchronize()
    got, how = out.cpu().numpy(), plan.last_plan()
    assert got.dtype == np.uint8 and got.shape == (frames_np.shape[0], plan.frame_bytes)
    plan.close()
    return got, how


@functools.lru_cache(maxsize=None)
def _images(size, deep):
    return model.images(size[0], size[1], "p010le" if deep else "nv12")


@functools.lru_cache(maxsize=None)
def _expected(size, layout, siting, matrix="bt601", rng="tv"):
    """The model's frames of _images(size, .): computed once, shared, never written to."""
    exp = np.stack([model.pack(f, layout, siting, matrix, rng) for f in _images(size, layout in model.DEEP)])
    exp.flags.writeable = False
    return exp


def _same(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape)
    bad = int((got != exp).sum())
    assert bad == 0, (what, bad)


# ---- frames equal the model ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("force_general", [False, True], ids=["default", "general"])
@pytest.mark.parametrize("siting", SITINGS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", SIZES, **ids)
def test_frames_equal_the_model(size, layout, siting, force_general):
    """Three frames (random, binary 0 / max, clamp colours plus greys) of: one pixel (all taps clamped), one block, odd edges both ways;
    4 x 8, one vec lane per row; 6 x 24, three lanes per row (the left-neighbour load across lanes and at a row start); 5 x 520, 65 lanes
    per row (a neighbour in another wave) with an odd height under vec; 37 x 131, the general path over more than one block.  The plan says
    vec exactly where w % 8 == 0 and nothing is forced, and always names the siting."""
    got, how = _run(_images(size, layout in model.DEEP), layout, siting, force_general)
    assert how == _name(layout, size[1] % 8 == 0 and not force_general, siting, 3), how
    _same(got, _expected(size, layout, siting), (size, how))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", SIZES, **ids)
def test_center_is_the_box_stage_on_the_device_and_left_is_not(size, layout):
    """The three frames through the EXISTING box plan of the layout on the device: "center" gives its bytes, on both paths; "left" differs
    from it on the four larger sizes (Y never does)."""
    import torch
    from pythoncrt_amd import formats
    frames = _images(size, layout in model.DEEP)
    old = formats.FORMATS[layout].egress(_dev(), size, layout=layout)
    ref = old(torch.from_numpy(frames).to(_dev())).cpu().numpy()
    old_how = old.last_plan()
    old.close()
    for force in (False, True):
        got, how = _run(frames, layout, "center", force)
        _same(got, ref, (size, how, old_how))
    left, how = _run(frames, layout, "left")
    if size in SIZES[4:]:
        h, w = size                                                  # the random frame
        a, b = model.samples(left[0], h, w, layout), model.samples(ref[0], h, w, layout)
        assert np.array_equal(a[0], b[0]), (how, old_how)
        differ = np.concatenate([(a[k] != b[k]).reshape(-1) for k in (1, 2)])
        print(how, old_how, "chroma samples that differ", float(differ.mean()))
        assert differ.mean() >= 0.5, (how, old_how, float(differ.mean()))


@pytest.mark.parametrize("force_general", [False, True], ids=["default", "general"])
@pytest.mark.parametrize("matrix,rng", model.CASES)
@pytest.mark.parametrize("size", [(37, 131), (6, 24)], **ids)
def test_every_matrix_and_range(size, matrix, rng, force_general):
    for layout in LAYOUTS:
        for siting in SITINGS:
            got, how = _run(_images(size, layout in model.DEEP), layout, siting, force_general, matrix=matrix, rng=rng)
            assert how == _name(layout, size[1] % 8 == 0 and not force_general, siting, 3), how
            _same(got, _expected(size, layout, siting, matrix, rng), (size, matrix, rng, how))


# ---- 10-bit: the quantiser and the bits outside a sample ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("force_general", [False, True], ids=["vec", "general"])
@pytest.mark.parametrize("layout", model.DEEP)
def test_every_half_bit_pattern_and_the_bits_outside_a_sample(layout, force_general):
    """144 x 160 x 3 = 69 120 samples in one frame: sample i of the flat half array has pattern i mod 65536 — NaNs of both kinds,
    infinities, negatives, -0, subnormals and every tie of the quantiser; a second frame has them in reversed order (so the filter mixes
    them otherwise).  Equal to the model bit for bit at both sitings, and the six bits of every word outside its sample are 0."""
    h, w = 144, 160
    pat = (np.arange(h * w * 3, dtype=np.int64) % 65536).astype(np.uint16)
    frames = np.stack([pat, pat[::-1]]).view(np.float16).reshape(2, h, w, 3)
    assert len(set(frames[0].view(np.uint16).reshape(-1).tolist())) == 65536
    for siting in SITINGS:
        got, how = _run(frames, layout, siting, force_general)
        assert how == _name(layout, not force_general, siting, 2), how
        _same(got, np.stack([model.pack(f, layout, siting) for f in frames]), how)
        words = deep_model.words(got)
        assert int((words & (0x003F if layout == "p010le" else 0xFC00)).sum()) == 0, how


# ---- the siting option on a live plan ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
def test_switching_the_siting_on_a_live_plan(layout):
    """set_option(SITING) back and forth on one plan, on both paths: each run gives the bytes of the model of that siting."""
    import torch
    from pythoncrt_amd import EgressSited
    from pythoncrt_amd._lib import CrtfxError
    size = (6, 24)
    deep = layout in model.DEEP
    src = torch.from_numpy(_images(size, deep)).to(_dev())
    plan = EgressSited(_dev(), size, layout)
    assert plan.siting == "left" and plan.last_plan() == _name(layout, True, "left", 0) and plan.plan()["siting"] == "left"
    for siting, force in (("center", False), ("left", False), ("center", True), ("center", False), ("left", True), ("left", False)):
        plan.siting = siting
        plan.force_general = force
        assert plan.siting == siting and plan.last_plan() == _name(layout, not force, siting, 0)
        got = plan(src).cpu().numpy()
        how = plan.last_plan()
        assert how == _name(layout, not force, siting, 3), how
        _same(got, _expected(size, layout, siting), how)
    plan.set_option(_lib.EGRESS_SITED_OPT_SITING, _lib.SITED_CENTER)
    assert plan.siting == "center"
    for option, value, word in ((_lib.EGRESS_SITED_OPT_SITING, 2, "SITING"), (_lib.EGRESS_SITED_OPT_SITING, -1, "SITING"),
                                (_lib.EGRESS_SITED_OPT_FORCE_GENERAL, 2, "FORCE_GENERAL"), (3, 0, "option"), (0, 1, "option")):
        with pytest.raises(CrtfxError) as e:
            plan.set_option(option, value)
        assert e.value.code == _lib.E_INVALID and word in str(e.value)
    assert plan.siting == "center" and plan.last_plan() == _name(layout, True, "center", 0)     # a refused option changes nothing
    with pytest.raises(ValueError):
        plan.siting = "top-left"
    wrong = torch.zeros((1,) + size + (3,), dtype=torch.uint8 if deep else torch.float16, device=_dev())
    with pytest.raises(CrtfxError) as e:                            # the other pixel format
        plan(wrong)
    assert e.value.code == _lib.E_UNSUPPORTED
    plan.close()


# ---- misaligned bases and strided batches ---------------------------------------------------------------------------------------------------

# (source offset, destination offset, source gap, destination gap, vec?)
STRIDES8 = [(0, 0, 8, 12, True), (4, 8, 4, 4, True), (1, 0, 4, 4, False), (0, 1, 4, 4, False), (2, 0, 4, 4, False), (0, 2, 4, 4, False),
            (0, 0, 3, 4, False), (0, 0, 4, 5, False), (0, 0, 2, 4, False), (3, 1, 1, 7, False)]
STRIDES10 = [(0, 0, 8, 12, True), (4, 8, 4, 4, True), (2, 0, 4, 4, False), (0, 2, 4, 4, False), (0, 0, 2, 4, False), (0, 0, 4, 6, False), (2, 6, 2, 2, False)]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_offset_and_strided_batches_leave_the_gaps_alone(layout):
    """n = 3 frames of 19 x 40 (an odd height under vec) that are slices of bigger sentinel-filled buffers on both sides, siting left.  A
    base that is no multiple of 4, or a stride that is none, takes general; multiples of 4 stay on vec.  Every frame right, every sentinel
    byte outside the frames untouched.  A 10-bit layout refuses an odd base or stride and writes nothing."""
    import torch
    from pythoncrt_amd import EgressSited
    size, n = (19, 40), 3
    deep = layout in model.DEEP
    src = _images(size, deep)
    exp = _expected(size, layout, "left")
    sbytes, dbytes = size[0] * size[1] * (6 if deep else 3), exp.shape[1]
    plan = EgressSited(_dev(), size, layout)
    for s_off, d_off, s_pad, d_pad, vec in (STRIDES10 if deep else STRIDES8):
        sbuf = torch.full((s_off + n * (sbytes + s_pad) + 16,), 0xEE, dtype=torch.uint8, device=_dev())
        dbuf = torch.full((d_off + n * (dbytes + d_pad) + 16,), 0x5A, dtype=torch.uint8, device=_dev())
        assert sbuf.data_ptr() % 4 == 0 and dbuf.data_ptr() % 4 == 0
        sview = sbuf[s_off:s_off + n * (sbytes + s_pad)].view(n, sbytes + s_pad)[:, :sbytes]
        dview = dbuf[d_off:d_off + n * (dbytes + d_pad)].view(n, dbytes + d_pad)[:, :dbytes]
        sview.copy_(torch.from_numpy(np.ascontiguousarray(src).view(np.uint8).reshape(n, sbytes)).to(_dev()))
        frames = (sview.view(torch.float16) if deep else sview).unflatten(1, size + (3,))
        assert plan(frames, out=dview) is dview
        torch.cuda.synchronize()
        how = plan.last_plan()
        assert how == _name(layout, vec, "left", 3), (how, s_off, d_off, s_pad, d_pad)
        _same(dview.cpu().numpy(), exp, (how, s_off, d_off, s_pad, d_pad))
        keep = torch.ones_like(dbuf, dtype=torch.bool)
        keep[d_off:d_off + n * (dbytes + d_pad)].view(n, dbytes + d_pad)[:, :dbytes] = False
        assert bool((dbuf[keep] == 0x5A).all()), (how, s_off, d_off)
    if deep:
        sbuf = torch.zeros((n * sbytes + 16,), dtype=torch.uint8, device=_dev())
        dbuf = torch.full((n * dbytes + 16,), 0x5A, dtype=torch.uint8, device=_dev())
        run, err, st = plan.lib.crtfx_egress_sited_run, plan.lib.crtfx_egress_sited_last_error, torch.cuda.current_stream().cuda_stream
        sp, dp = sbuf.data_ptr(), dbuf.data_ptr()
        for args in ((sp + 1, sbytes, dp, dbytes), (sp, sbytes, dp + 1, dbytes), (sp, sbytes + 1, dp, dbytes), (sp, sbytes, dp, dbytes + 1)):
            assert run(plan._plan, args[0], args[1], args[2], args[3], 2, st) == _lib.E_INVALID and b"odd" in err(plan._plan), (plan.last_plan(), args)
        torch.cuda.synchronize()
        assert bool((dbuf == 0x5A).all()), plan.last_plan()
    assert tuple(plan.planes(dview)[0].shape) == (n,) + size
    plan.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_call_is_run_and_batches_may_be_slices(layout):
    """plan(x) == plan.run(x); frames 1..2 of a batch of four, written into rows 1..2 of a larger output, touch nothing else."""
    import torch
    from pythoncrt_amd import EgressSited
    size = (6, 24)
    deep = layout in model.DEEP
    imgs = _images(size, deep)
    big = torch.from_numpy(np.concatenate([imgs, imgs[:1]])).to(_dev())
    plan = EgressSited(_dev(), size, layout)
    a, b = plan(big[:3]).cpu().numpy(), plan.run(big[:3]).cpu().numpy()
    _same(a, b, plan.last_plan())
    out = torch.full((4, plan.frame_bytes), 0x5A, dtype=torch.uint8, device=_dev())
    assert plan.run(big[1:3], out=out[1:3]).data_ptr() == out[1:3].data_ptr()
    got = out.cpu().numpy()
    _same(got[1:3], _expected(size, layout, "left")[1:3], plan.last_plan())
    assert (got[0] == 0x5A).all() and (got[3] == 0x5A).all()
    plan.close()


@pytest.mark.parametrize("layout", ["nv12", "uyvy422", "p010le"])
def test_one_batch_at_1080p(layout):
    """2 frames of 1080 x 1920 per family, on the vec path, siting left."""
    size = (1080, 1920)
    rs = np.random.default_rng(1080)
    if layout in model.DEEP:
        frames = (rs.integers(0, 2048, (2,) + size + (3,)) / 8.0).astype(np.float16)       # eighths: ties of the quantiser among them
    else:
        frames = rs.integers(0, 256, (2,) + size + (3,), dtype=np.uint8)
    got, how = _run(frames, layout, "left")
    assert how == _name(layout, True, "left", 2), how
    for i in range(2):
        _same(got[i], model.pack(frames[i], layout, "left"), (how, i))


# ---- process_frames -----------------------------------------------------------------------------------------------------------------------

def _spy(monkeypatch, cls, log):
    """Record the plan string of every run of a plan class."""
    inner = cls.run

    def run(self, frames, out=None):
        res = inner(self, frames, out)
        log.append(self.last_plan())
        return res
    monkeypatch.setattr(cls, "run", run)


def _render(frames, w, h, **kw):
    import pythoncrt_amd as pc
    got = []
    assert pc.process_frames(iter(frames), lambda a: got.append(np.array(a)), w, h, 30.0, len(frames), **kw) == len(frames)
    return got


@pytest.mark.parametrize("layout", ["nv12", "uyvy422"])
def test_process_frames_left_is_the_model_of_its_rgb24_frames(monkeypatch, layout):
    """Five 36 x 64 frames in batches of 2, the grain fixed by noise_seed: with out_chroma="left" the writer gets the model applied to the
    rgb24 frames of the same call."""
    import pythoncrt_amd as pc
    h, w, n = 36, 64, 5
    kw = dict(noise_seed=9, batch=2, persistence=0.3)
    frames = np.random.default_rng(61).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    rgb = _render(frames, w, h, **kw)
    log = []
    _spy(monkeypatch, pc.EgressSited, log)
    got = _render(frames, w, h, out_pix_fmt=layout, out_matrix="bt709", out_range="pc", out_chroma="left", **kw)
    assert log == [_name(layout, True, "left", k) for k in (2, 2, 1)], log
    fb = model.frame_bytes(h, w, layout)
    for i in range(n):
        assert got[i].shape == (fb,) and got[i].dtype == np.uint8
        _same(got[i], model.pack(rgb[i], layout, "left", "bt709", "pc"), (log, i))
    assert not np.array_equal(rgb[0], rgb[1])


def test_process_frames_left_on_both_ends_of_the_half_chain(monkeypatch):
    """Five 36 x 64 frames, batch 2: p010le in with in_chroma="left", yuv420p10le out with out_chroma="left" — the writer gets the egress
    model of FramePipeline(dtype=float16) run batch by batch on the sited source model's RGB."""
    import torch
    import pythoncrt_amd as pc
    from pythoncrt_amd.pipeline import FramePipeline, RenderSettings
    from tests import sited_model
    h, w, n = 36, 64, 5
    fb = deep_model.sizes(h, w)[2]
    src = deep_model.to_bytes(np.random.default_rng(62).integers(0, 1024, (n, fb // 2)).astype(np.uint16) << 6).reshape(n, fb)
    rgb = torch.from_numpy(np.stack([sited_model.unpack(p, h, w, "p010le", "left") for p in src])).to(_dev())
    pipe = FramePipeline(_dev(), h, w, RenderSettings(), fps=30.0, noise_seed=9, dtype=torch.float16)
    state, outs = None, []
    for i in range(0, n, 2):
        out, state = pipe.run(rgb[i:i + 2], first_index=i, state=state)
        outs.append(out.cpu().numpy())
    exp = np.stack([model.pack(f, "yuv420p10le", "left") for f in np.concatenate(outs)])
    log_in, log_out = [], []
    _spy(monkeypatch, pc.UnpackSited, log_in)
    _spy(monkeypatch, pc.EgressSited, log_out)
    got = _render(src, w, h, noise_seed=9, batch=2, in_pix_fmt="p010le", out_pix_fmt="yuv420p10le", in_chroma="left", out_chroma="left")
    assert log_out == [_name("yuv420p10le", True, "left", k) for k in (2, 2, 1)] and len(log_in) == 3, (log_in, log_out)
    _same(np.stack(got), exp, log_out)


def test_process_frames_center_is_the_path_as_it_was(monkeypatch):
    """out_chroma="center", spelled out or left out: the box plan, its plan string and its bytes (tests/yuv_model.py)."""
    import pythoncrt_amd as pc
    from tests import yuv_model
    h, w, n = 36, 64, 3
    kw = dict(noise_seed=9, batch=2)
    frames = np.random.default_rng(63).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    rgb = _render(frames, w, h, **kw)
    log, sited_log = [], []
    _spy(monkeypatch, pc.EgressYuv, log)
    _spy(monkeypatch, pc.EgressSited, sited_log)
    for extra in (dict(out_chroma="center"), {}):
        got = _render(frames, w, h, out_pix_fmt="nv12", **extra, **kw)
        for i in range(n):
            _same(got[i], yuv_model.pack(rgb[i], "nv12"), (log, i))
    assert log == ["egress=k_egress_420<nv12,vec>;frames=2", "egress=k_egress_420<nv12,vec>;frames=1"] * 2 and not sited_log, (log, sited_log)


# ---- CLI ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("io", ["staged", "mapped"])
def test_cli_out_chroma_left(tmp_path, monkeypatch, io):
    """--out-pix-fmt nv12 --out-chroma left over a 3-frame 36 x 64 file (batch 2), --io staged and --io mapped: the output file equals the
    model of the CLI's own rgb24 run of the same flags and seed."""
    import pythoncrt_amd as pc
    from pythoncrt_amd import cli
    n, h, w = 3, 36, 64
    frames = np.random.default_rng(64).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    (tmp_path / "in.rgb").write_bytes(frames.tobytes())
    flags = ["--input", str(tmp_path / "in.rgb"), "--width", str(w), "--height", str(h), "--fps", "30", "--batch", "2", "--noise-seed", "17",
             "--persistence", "0.3", "--io", io]
    log = []
    _spy(monkeypatch, pc.EgressSited, log)
    assert cli.main(flags + ["--output", str(tmp_path / "out.rgb")]) == 0
    assert cli.main(flags + ["--output", str(tmp_path / "out.nv12"), "--out-pix-fmt", "nv12", "--out-matrix", "bt709", "--out-chroma", "left"]) == 0
    rgb = np.frombuffer((tmp_path / "out.rgb").read_bytes(), dtype=np.uint8).reshape(n, h, w, 3)
    fb = model.frame_bytes(h, w, "nv12")
    raw = (tmp_path / "out.nv12").read_bytes()
    assert log == [_name("nv12", True, "left", k) for k in (2, 1)], log
    assert len(raw) == n * fb
    got = np.frombuffer(raw, dtype=np.uint8).reshape(n, fb)
    for i in range(n):
        _same(got[i], model.pack(rgb[i], "nv12", "left", "bt709", "tv"), (io, log, i))
    assert not np.array_equal(rgb[0], rgb[1])
