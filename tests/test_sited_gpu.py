"""The sited source stage on the GPU: UnpackSited (k_unpack_sited, seven layouts x vec / general, siting left / center) against the int64
host model of tests/sited_model.py — equality is zero differing elements, and every assert names the plan string — against the replicating
stages for the same input (the taps are live), and process_frames / the CLI with in_chroma against the rgb24 run fed the model's RGB."""
import functools

import numpy as np
import pytest

from pythoncrt_amd import _lib
from tests import deep_model
from tests import sited_model as model

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (2, 2), (3, 5), (5, 3), (4, 8), (6, 24), (5, 520), (37, 131)]
LAYOUTS = list(model.LAYOUTS)
SITINGS = list(model.SITINGS)
ids = dict(ids=lambda s: f"{s[0]}x{s[1]}")


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _name(layout, vec, siting, frames):
    return f"sited=k_unpack_sited<{layout},{'vec' if vec else 'general'}>;siting={siting};frames={frames}"


def _bits(a):
    return a.view(np.uint16) if a.dtype == np.float16 else a


def _run(packed_np, size, layout, siting="left", force_general=False, matrix="bt601", rng="tv"):
    """(RGB [n, h, w, 3] from the device, last_plan) for a stack of packed frames."""
    import torch
    from pythoncrt_amd import UnpackSited
    plan = UnpackSited(_dev(), size, layout, matrix=matrix, range=rng, siting=siting, force_general=force_general)
    assert plan.siting == siting and plan.force_general == force_general and plan.frame_bytes == model.frame_bytes(size[0], size[1], layout)
    out = plan(torch.from_numpy(packed_np).to(_dev()))
    torch.cuda.synchronize()
    got, how = out.cpu().numpy(), plan.last_plan()
    assert got.dtype == (np.float16 if layout in model.DEEP else np.uint8) and got.shape == (packed_np.shape[0],) + tuple(size) + (3,)
    plan.close()
    return got, how


@functools.lru_cache(maxsize=None)
def _images(size, layout):
    return model.images(size[0], size[1], layout)


@functools.lru_cache(maxsize=None)
def _expected(size, layout, siting, matrix="bt601", rng="tv"):
    """The model's frames of _images(size, layout): computed once, shared, never written to."""
    exp = np.stack([model.unpack(p, size[0], size[1], layout, siting, matrix, rng) for p in _images(size, layout)])
    exp.flags.writeable = False
    return exp


def _same(got, exp, what):
    bad = int((_bits(got) != _bits(exp)).sum())
    assert got.shape == exp.shape and got.dtype == exp.dtype and bad == 0, (what, bad)


# ---- frames equal the model ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("force_general", [False, True], ids=["default", "general"])
@pytest.mark.parametrize("siting", SITINGS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", SIZES, **ids)
def test_frames_equal_the_model(size, layout, siting, force_general):
    """Three frames (random, binary 0 / max, clamp colours plus greys) of: one pixel, one block, odd edges with clamped taps both ways;
    4 x 8, one vec lane per row (both horizontal neighbours clamped); 6 x 24, three lanes per row (a lane's neighbour lane is another
    row's); 5 x 520, 65 lanes per row (a neighbour in another wave) with an odd height under vec; 37 x 131, the general path over more than
    one block.  The plan says vec exactly where w % 8 == 0 and nothing is forced, and always names the siting."""
    got, how = _run(_images(size, layout), size, layout, siting, force_general)
    assert how == _name(layout, size[1] % 8 == 0 and not force_general, siting, 3), how
    _same(got, _expected(size, layout, siting), (size, how))


@pytest.mark.parametrize("siting", SITINGS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", SIZES[4:], **ids)
def test_the_taps_are_live(size, layout, siting):
    """The random frame against the REPLICATING stage's result for the same input, from the device.  Where a pixel has a tap on another
    sample than its own (model.live: the tap tables), at least half of the elements differ; where it has none, all are equal.  At least
    half of the WHOLE frame differs from 6 x 24 up for every 4:2:0 layout and for siting "center" (the model alone shows 59 - 75 %).  Not
    asked of the whole frame: siting "left" on 4:2:2 — its even columns have the one tap (4, 0) and no vertical one, so they equal the
    replicating stage by the arithmetic itself and the frame can never reach one half (the model: 30 - 39 %) — and 4 x 8, where the clamped
    first and last rows leave a quarter of a 4:2:0 "left" frame without a second tap (the model: 49 - 66 %)."""
    import torch
    from pythoncrt_amd import formats
    packed = _images(size, layout)[:1]
    got, how = _run(packed, size, layout, siting)
    old = formats.FORMATS[layout].source(_dev(), size, layout=layout)
    ref = old(torch.from_numpy(packed).to(_dev())).cpu().numpy()
    what = (how, old.last_plan())
    old.close()
    each = _bits(got[0]) != _bits(ref[0])
    mask = model.live(size[0], size[1], layout, siting)
    print(what, "whole", float(each.mean()), "live", float(each[mask].mean()))
    assert not each[~mask].any() and each[mask].mean() >= 0.5, (what, float(each[mask].mean()))
    if size != (4, 8) and (layout in model.V420 or siting == "center"):
        assert each.mean() >= 0.5, (what, float(each.mean()))


@pytest.mark.parametrize("force_general", [False, True], ids=["default", "general"])
@pytest.mark.parametrize("matrix,rng", model.CASES)
@pytest.mark.parametrize("size", [(37, 131), (6, 24)], **ids)
def test_every_matrix_and_range(size, matrix, rng, force_general):
    for layout in LAYOUTS:
        for siting in SITINGS:
            got, how = _run(_images(size, layout), size, layout, siting, force_general, matrix=matrix, rng=rng)
            assert how == _name(layout, size[1] % 8 == 0 and not force_general, siting, 3), how
            _same(got, _expected(size, layout, siting, matrix, rng), (size, matrix, rng, how))


@pytest.mark.parametrize("force_general", [False, True], ids=["default", "general"])
@pytest.mark.parametrize("layout", model.DEEP)
def test_all_1024_codes_with_random_ignored_bits(layout, force_general):
    """64 x 64: the Y plane holds every 10-bit code four times, U and V each once, in shuffled orders; the six bits of every word outside
    its sample are random and change nothing."""
    h, w = 64, 64
    rs = np.random.default_rng(1024)
    y = np.concatenate([rs.permutation(1024) for _ in range(4)]).reshape(h, w)
    u, v = rs.permutation(1024).reshape(32, 32), rs.permutation(1024).reshape(32, 32)
    clean = deep_model.pack_planes(y, u, v, layout)
    junk = rs.integers(0, 64, clean.size // 2).astype(np.uint16)
    dirty = deep_model.to_bytes(deep_model.words(clean) | (junk if layout == "p010le" else junk << 10))
    assert not np.array_equal(dirty, clean) and all(np.array_equal(a, b) for a, b in zip(deep_model.planes(dirty, h, w, layout), (y, u, v)))
    for siting in SITINGS:
        exp = model.unpack(clean, h, w, layout, siting)
        got, how = _run(np.stack([dirty, clean]), (h, w), layout, siting, force_general)
        assert how == _name(layout, not force_general, siting, 2), how
        _same(got[0], exp, ("dirty", how))
        _same(got[1], exp, ("clean", how))


def test_a_matrix_at_the_admission_boundary_saturates_as_the_model_clamps():
    """10-bit: the largest luma and chroma coefficients crtfx_sited_create admits at offsets (64, 512, 512), signs chosen so that the sum of
    the two int32 parts passes int32 both ways: the saturating add gives the int64 model's codes."""
    import ctypes
    import torch
    from pythoncrt_amd import tables
    lib = _lib.load()
    l10, c10 = (2 ** 31 - 1) // (16 * 959), (2 ** 31 - 2 ** 19 - 1) // 8192
    m = np.array([[l10, c10, 0], [l10, -c10, 0], [-l10, 0, -c10]], dtype=np.int64)
    off = (64, 512, 512)
    h, w = 6, 24
    for layout in model.DEEP:
        packed = _images((h, w), layout)
        assert 16 * 959 * l10 + 8192 * c10 >= 2 ** 31                                           # what the corners of the cube reach
        for force in (0, 1):
            plan = ctypes.c_void_p()
            mi, oi = np.ascontiguousarray(m.reshape(-1), dtype=np.int32), np.ascontiguousarray(off, dtype=np.int32)
            assert lib.crtfx_sited_create(_dev().index, h, w, _lib.PIX_F16, model.LAYOUTS.index(layout), tables.ptr(mi), tables.ptr(oi), ctypes.byref(plan)) == _lib.OK
            assert lib.crtfx_sited_set_option(plan, _lib.SITED_OPT_FORCE_GENERAL, force) == _lib.OK
            src = torch.from_numpy(packed).to(_dev())
            dst = torch.empty((3, h, w, 3), dtype=torch.float16, device=_dev())
            assert lib.crtfx_sited_run(plan, src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0) * 2, 3, torch.cuda.current_stream().cuda_stream) == _lib.OK
            torch.cuda.synchronize()
            buf = ctypes.create_string_buffer(128)
            assert lib.crtfx_sited_last_plan(plan, buf, 128) == _lib.OK
            how = buf.value.decode()
            assert how == _name(layout, not force, "left", 3), how
            exp = np.stack([model.unpack(p, h, w, layout, "left", m=m, off=off) for p in packed])
            _same(dst.cpu().numpy(), exp, how)
            assert lib.crtfx_sited_destroy(plan) == _lib.OK


# ---- the siting option on a live plan ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
def test_switching_the_siting_on_a_live_plan(layout):
    """set_option(SITING) back and forth on one plan, on both paths: each run gives the bytes of a fresh plan of that siting (the model's)."""
    import torch
    from pythoncrt_amd import UnpackSited
    from pythoncrt_amd._lib import CrtfxError
    size = (6, 24)
    src = torch.from_numpy(_images(size, layout)).to(_dev())
    plan = UnpackSited(_dev(), size, layout)
    assert plan.siting == "left" and plan.last_plan() == _name(layout, True, "left", 0) and plan.plan()["siting"] == "left"
    for siting, force in (("center", False), ("left", False), ("center", True), ("center", False), ("left", True), ("left", False)):
        plan.siting = siting
        plan.force_general = force
        assert plan.siting == siting and plan.last_plan() == _name(layout, not force, siting, 0)
        got = plan(src).cpu().numpy()
        how = plan.last_plan()
        assert how == _name(layout, not force, siting, 3), how
        _same(got, _expected(size, layout, siting), how)
        fresh, fresh_how = _run(_images(size, layout), size, layout, siting, force)
        _same(got, fresh, (how, fresh_how))
    plan.set_option(_lib.SITED_OPT_SITING, _lib.SITED_CENTER)
    assert plan.siting == "center"
    for option, value, word in ((_lib.SITED_OPT_SITING, 2, "SITING"), (_lib.SITED_OPT_SITING, -1, "SITING"), (_lib.SITED_OPT_FORCE_GENERAL, 2, "FORCE_GENERAL"),
                                (3, 0, "option"), (0, 1, "option")):
        with pytest.raises(CrtfxError) as e:
            plan.set_option(option, value)
        assert e.value.code == _lib.E_INVALID and word in str(e.value)
    assert plan.siting == "center" and plan.last_plan() == _name(layout, True, "center", 0)     # a refused option changes nothing
    with pytest.raises(ValueError):
        plan.siting = "top-left"
    plan.close()


# ---- misaligned bases and strided batches ---------------------------------------------------------------------------------------------------

# (source offset, destination offset, source gap, destination gap, vec?)
STRIDES8 = [(0, 0, 8, 12, True), (4, 8, 4, 4, True), (1, 0, 4, 4, False), (0, 1, 4, 4, False), (2, 0, 4, 4, False), (0, 2, 4, 4, False),
            (0, 0, 3, 4, False), (0, 0, 4, 5, False), (0, 0, 2, 4, False), (3, 1, 1, 7, False)]
STRIDES10 = [(0, 0, 8, 12, True), (4, 8, 4, 4, True), (2, 0, 4, 4, False), (0, 2, 4, 4, False), (0, 0, 2, 4, False), (0, 0, 4, 6, False), (2, 6, 2, 2, False)]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_offset_and_strided_batches_leave_the_gaps_alone(layout):
    """n = 3 frames of 19 x 40 that are slices of bigger sentinel-filled buffers on both sides, siting center.  A base that is no multiple
    of 4, or a stride that is none, takes general; multiples of 4 stay on vec.  Every frame right, every sentinel byte outside the frames
    untouched.  A 10-bit layout refuses an odd base or stride and writes nothing."""
    import torch
    from pythoncrt_amd import UnpackSited
    size, n = (19, 40), 3
    deep = layout in model.DEEP
    src = _images(size, layout)
    exp = _expected(size, layout, "center")
    sbytes, dbytes = src.shape[1], size[0] * size[1] * (6 if deep else 3)
    plan = UnpackSited(_dev(), size, layout, siting="center")
    for s_off, d_off, s_pad, d_pad, vec in (STRIDES10 if deep else STRIDES8):
        sbuf = torch.full((s_off + n * (sbytes + s_pad) + 16,), 0xEE, dtype=torch.uint8, device=_dev())
        dbuf = torch.full((d_off + n * (dbytes + d_pad) + 16,), 0x5A, dtype=torch.uint8, device=_dev())
        assert sbuf.data_ptr() % 4 == 0 and dbuf.data_ptr() % 4 == 0
        sview = sbuf[s_off:s_off + n * (sbytes + s_pad)].view(n, sbytes + s_pad)[:, :sbytes]
        dview = dbuf[d_off:d_off + n * (dbytes + d_pad)].view(n, dbytes + d_pad)[:, :dbytes]
        sview.copy_(torch.from_numpy(src).to(_dev()))
        out = (dview.view(torch.float16) if deep else dview).unflatten(1, size + (3,))
        assert plan(sview, out=out) is out
        torch.cuda.synchronize()
        how = plan.last_plan()
        assert how == _name(layout, vec, "center", 3), (how, s_off, d_off, s_pad, d_pad)
        _same(out.cpu().numpy(), exp, (how, s_off, d_off, s_pad, d_pad))
        keep = torch.ones_like(dbuf, dtype=torch.bool)
        keep[d_off:d_off + n * (dbytes + d_pad)].view(n, dbytes + d_pad)[:, :dbytes] = False
        assert bool((dbuf[keep] == 0x5A).all()), (how, s_off, d_off)
    if deep:
        sbuf = torch.zeros((n * sbytes + 16,), dtype=torch.uint8, device=_dev())
        dbuf = torch.full((n * dbytes + 16,), 0x5A, dtype=torch.uint8, device=_dev())
        run, err, st = plan.lib.crtfx_sited_run, plan.lib.crtfx_sited_last_error, torch.cuda.current_stream().cuda_stream
        sp, dp = sbuf.data_ptr(), dbuf.data_ptr()
        for args in ((sp + 1, sbytes, dp, dbytes), (sp, sbytes, dp + 1, dbytes), (sp, sbytes + 1, dp, dbytes), (sp, sbytes, dp, dbytes + 1)):
            assert run(plan._plan, args[0], args[1], args[2], args[3], 2, st) == _lib.E_INVALID and b"odd" in err(plan._plan), (plan.last_plan(), args)
        torch.cuda.synchronize()
        assert bool((dbuf == 0x5A).all()), plan.last_plan()
    assert tuple(plan.planes(sview)[0].shape) == (n,) + size
    plan.close()


@pytest.mark.parametrize("layout,siting", [("nv12", "left"), ("uyvy422", "center"), ("p010le", "left")])
def test_one_batch_at_1080p(layout, siting):
    """2 frames of 1080 x 1920 per family, on the vec path."""
    size = (1080, 1920)
    fb = model.frame_bytes(size[0], size[1], layout)
    rs = np.random.default_rng(1080)
    if layout in model.DEEP:
        packed = deep_model.to_bytes(rs.integers(0, 1024, (2, fb // 2)).astype(np.uint16) << 6).reshape(2, fb)
    else:
        packed = rs.integers(0, 256, (2, fb), dtype=np.uint8)
    got, how = _run(packed, size, layout, siting)
    assert how == _name(layout, True, siting, 2), how
    for i in range(2):
        _same(got[i], model.unpack(packed[i], size[0], size[1], layout, siting), (how, i))


# ---- process_frames -----------------------------------------------------------------------------------------------------------------------

def _render_rgb24(frames, w, h, **kw):
    """What process_frames writes for rgb24 in and out: uint8 [n, h, w, 3]."""
    import pythoncrt_amd as pc
    got = []
    assert pc.process_frames(iter(frames), lambda a: got.append(np.array(a)), w, h, 30.0, len(frames), **kw) == len(frames)
    return np.stack(got)


def _spy(monkeypatch, cls, log):
    """Record the plan string of every run of a source plan class."""
    inner = cls.run

    def run(self, packed, out=None):
        res = inner(self, packed, out)
        log.append(self.last_plan())
        return res
    monkeypatch.setattr(cls, "run", run)


def _sources(h, w, layout, n, seed):
    fb = model.frame_bytes(h, w, layout)
    return np.random.default_rng(seed).integers(0, 256, (n, fb), dtype=np.uint8)


@pytest.mark.parametrize("layout,siting", [("nv12", "left"), ("uyvy422", "center")])
def test_process_frames_interpolates_an_8_bit_source(monkeypatch, layout, siting):
    """Five 36 x 64 frames in batches of 2, the grain fixed by noise_seed: in_chroma=siting equals the rgb24 path fed the model's RGB."""
    import pythoncrt_amd as pc
    h, w, n = 36, 64, 5
    kw = dict(noise_seed=9, batch=2, persistence=0.3)
    src = _sources(h, w, layout, n, 51)
    rgb = np.stack([model.unpack(p, h, w, layout, siting, "bt709", "pc") for p in src])
    ref = _render_rgb24(rgb, w, h, **kw)
    log, got = [], []
    _spy(monkeypatch, pc.UnpackSited, log)
    assert pc.process_frames(iter(src), lambda a: got.append(np.array(a)), w, h, 30.0, n, in_pix_fmt=layout, in_matrix="bt709", in_range="pc",
                             in_chroma=siting, **kw) == n
    assert log == [_name(layout, True, siting, k) for k in (2, 2, 1)], log
    _same(np.stack(got), ref, log)


def test_process_frames_resizes_an_off_size_sited_source(monkeypatch):
    """An 18 x 32 yuv420p source for a 36 x 64 output: UnpackSited stands in front of IngestResize; the frames equal the rgb24 run fed the
    model's RGB with resize_on="device"."""
    import pythoncrt_amd as pc
    h, w, sh, sw, n = 36, 64, 18, 32, 3
    kw = dict(noise_seed=5, batch=2)
    src = _sources(sh, sw, "yuv420p", n, 52)
    ref = _render_rgb24(np.stack([model.unpack(p, sh, sw, "yuv420p", "left") for p in src]), w, h, resize_on="device", **kw)
    log, got = [], []
    _spy(monkeypatch, pc.UnpackSited, log)
    assert pc.process_frames(iter(src), lambda a: got.append(np.array(a)), w, h, 30.0, n, in_pix_fmt="yuv420p", in_size=(sh, sw), in_chroma="left", **kw) == n
    assert log == [_name("yuv420p", True, "left", k) for k in (2, 1)], log
    _same(np.stack(got), ref, log)


def test_process_frames_interpolates_in_front_of_the_half_chain(monkeypatch):
    """Four 72 x 320 frames in one batch, p010le in / yuv420p10le out, in_chroma="center": the writer gets
    deep_model.pack(FramePipeline(dtype=float16).run(the model's RGB)), byte for byte."""
    import torch
    import pythoncrt_amd as pc
    from pythoncrt_amd.pipeline import FramePipeline, RenderSettings
    h, w, n = 72, 320, 4
    fb = deep_model.sizes(h, w)[2]
    src = deep_model.to_bytes(np.random.default_rng(53).integers(0, 1024, (n, fb // 2)).astype(np.uint16) << 6).reshape(n, fb)
    rgb = torch.from_numpy(np.stack([model.unpack(p, h, w, "p010le", "center") for p in src])).to(_dev())
    pipe = FramePipeline(_dev(), h, w, RenderSettings(), fps=30.0, noise_seed=9, dtype=torch.float16)
    out, _ = pipe.run(rgb, first_index=0, state=None)
    torch.cuda.synchronize()
    exp = np.stack([deep_model.pack(f, "yuv420p10le") for f in out.cpu().numpy()])
    log, got = [], []
    _spy(monkeypatch, pc.UnpackSited, log)
    assert pc.process_frames(iter(src), lambda a: got.append(np.array(a)), w, h, 30.0, n, noise_seed=9, batch=4, in_pix_fmt="p010le",
                             out_pix_fmt="yuv420p10le", in_chroma="center") == n
    assert log == [_name("p010le", True, "center", 4)], log
    _same(np.stack(got), exp, log)


def test_process_frames_replicate_is_the_path_as_it_was(monkeypatch):
    """in_chroma="replicate", spelled out or left out: the replicating plan, its plan string and its bytes (tests/unpack_model.py)."""
    import pythoncrt_amd as pc
    from tests import unpack_model
    h, w, n = 36, 64, 3
    kw = dict(noise_seed=9, batch=2)
    src = _sources(h, w, "nv12", n, 54)
    ref = _render_rgb24(np.stack([unpack_model.unpack(p, h, w, "nv12") for p in src]), w, h, **kw)
    log, sited_log = [], []
    _spy(monkeypatch, pc.UnpackYuv, log)
    _spy(monkeypatch, pc.UnpackSited, sited_log)
    for extra in (dict(in_chroma="replicate"), {}):
        got = []
        assert pc.process_frames(iter(src), lambda a: got.append(np.array(a)), w, h, 30.0, n, in_pix_fmt="nv12", **extra, **kw) == n
        _same(np.stack(got), ref, log)
    assert log == ["unpack=k_unpack_420<nv12,vec>;frames=2", "unpack=k_unpack_420<nv12,vec>;frames=1"] * 2 and not sited_log, (log, sited_log)


# ---- CLI ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("io", ["staged", "mapped"])
def test_cli_in_chroma_left(tmp_path, monkeypatch, io):
    """--in-pix-fmt nv12 --in-chroma left over a 3-frame 36 x 64 file (batch 2), --io staged and --io mapped: the output file equals the
    CLI's own rgb24 run of the same flags and seed on the model's RGB."""
    import pythoncrt_amd as pc
    from pythoncrt_amd import cli
    n, h, w = 3, 36, 64
    src = _sources(h, w, "nv12", n, 55)
    (tmp_path / "in.nv12").write_bytes(src.tobytes())
    (tmp_path / "in.rgb").write_bytes(np.stack([model.unpack(p, h, w, "nv12", "left", "bt709", "tv") for p in src]).tobytes())
    flags = ["--width", str(w), "--height", str(h), "--fps", "30", "--batch", "2", "--noise-seed", "17", "--persistence", "0.3", "--io", io]
    log = []
    _spy(monkeypatch, pc.UnpackSited, log)
    assert cli.main(flags + ["--input", str(tmp_path / "in.nv12"), "--output", str(tmp_path / "out.a"), "--in-pix-fmt", "nv12", "--in-matrix", "bt709",
                             "--in-chroma", "left"]) == 0
    assert cli.main(flags + ["--input", str(tmp_path / "in.rgb"), "--output", str(tmp_path / "out.b")]) == 0
    got = np.frombuffer((tmp_path / "out.a").read_bytes(), dtype=np.uint8)
    ref = np.frombuffer((tmp_path / "out.b").read_bytes(), dtype=np.uint8)
    assert log == [_name("nv12", True, "left", k) for k in (2, 1)], log
    assert got.size == n * h * w * 3
    _same(got, ref, (io, log))
    assert not np.array_equal(ref.reshape(n, -1)[0], ref.reshape(n, -1)[1])
