"""The field-paired 4:2:0 source stage on the GPU: UnpackField420 (k_unpack_field420, four layouts x vec / general, chroma replicate / left /
center) against the int64 host model of tests/field420_model.py — equality is zero differing elements, and every assert names the plan
string — and, for "replicate", against the existing replicating plans run on each field on the device."""
import ctypes
import functools

import numpy as np
import pytest

from pythoncrt_amd import _lib
from tests import deep_model
from tests import field420_model as model

pytestmark = pytest.mark.gpu

# widths narrower than a lane's block, w % 8 zero and non-zero, h % 4 of 0 and 2, one and several lane rows (16 x 136: 17 lanes to a row)
SIZES = [(4, 1), (4, 2), (4, 8), (6, 7), (8, 16), (10, 24), (12, 40), (22, 72), (16, 136)]
LAYOUTS = list(model.LAYOUTS)
CHROMAS = list(model.CHROMAS)
ids = dict(ids=lambda s: f"{s[0]}x{s[1]}")


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _name(layout, vec, chroma, frames):
    return f"field420=k_unpack_field420<{layout},{'vec' if vec else 'general'}>;chroma={chroma};frames={frames}"


def _bits(a):
    return a.view(np.uint16) if a.dtype == np.float16 else a


def _run(packed_np, size, layout, chroma="replicate", force_general=False, matrix="bt601", rng="tv"):
    """(RGB [n, h, w, 3] from the device, last_plan) for a stack of packed frames."""
    import torch
    from pythoncrt_amd import UnpackField420
    plan = UnpackField420(_dev(), size, layout, matrix=matrix, range=rng, chroma=chroma, force_general=force_general)
    assert plan.chroma == chroma and plan.force_general == force_general and plan.frame_bytes == model.frame_bytes(size[0], size[1], layout)
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
def _expected(size, layout, chroma, matrix="bt601", rng="tv"):
    """The model's frames of _images(size, layout): computed once, shared, never written to."""
    exp = model.unpack_batch(_images(size, layout), size[0], size[1], layout, chroma, matrix, rng)
    exp.flags.writeable = False
    return exp


def _same(got, exp, what):
    bad = int((_bits(got) != _bits(exp)).sum())
    assert got.shape == exp.shape and got.dtype == exp.dtype and bad == 0, (what, bad)


# ---- frames equal the model ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("force_general", [False, True], ids=["default", "general"])
@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", SIZES, **ids)
def test_frames_equal_the_model(size, layout, chroma, force_general):
    """Batches of 1, 2 and 3 frames (random, binary 0 / max, clamp colours plus greys).  The plan says vec exactly where w % 8 == 0 and
    nothing is forced, and always names the chroma."""
    for n in (1, 2, 3):
        got, how = _run(_images(size, layout)[:n], size, layout, chroma, force_general)
        assert how == _name(layout, size[1] % 8 == 0 and not force_general, chroma, n), how
        _same(got, _expected(size, layout, chroma)[:n], (size, how))


@pytest.mark.parametrize("force_general", [False, True], ids=["default", "general"])
@pytest.mark.parametrize("matrix,rng", model.CASES)
def test_every_matrix_and_range(matrix, rng, force_general):
    size = (10, 24)
    for layout in LAYOUTS:
        for chroma in CHROMAS:
            got, how = _run(_images(size, layout), size, layout, chroma, force_general, matrix=matrix, rng=rng)
            assert how == _name(layout, not force_general, chroma, 3), how
            _same(got, _expected(size, layout, chroma, matrix, rng), (matrix, rng, how))


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
    for chroma in CHROMAS:
        exp = model.unpack(clean, h, w, layout, chroma)
        got, how = _run(np.stack([dirty, clean]), (h, w), layout, chroma, force_general)
        assert how == _name(layout, not force_general, chroma, 2), how
        _same(got[0], exp, ("dirty", how))
        _same(got[1], exp, ("clean", how))


@pytest.mark.parametrize("force_general", [False, True], ids=["default", "general"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", [(8, 16), (12, 40), (16, 7)], **ids)
def test_replicate_is_the_existing_plans_run_on_each_field(size, layout, force_general):
    """h % 4 == 0: the device's frames against the family's replicating plan run, on the device, on each field as an h/2 x w frame of its
    own, the two results woven."""
    import torch
    from pythoncrt_amd import formats
    h, w = size
    packed = _images(size, layout)
    got, how = _run(packed, size, layout, "replicate", force_general)
    old = formats.FORMATS[layout].source(_dev(), (h // 2, w), layout=layout)
    exp = np.empty_like(got)
    for f in (0, 1):
        fields = np.stack([model.field_frame(p, h, w, layout, f) for p in packed])
        exp[:, f::2] = old(torch.from_numpy(fields).to(_dev())).cpu().numpy()
    what = (how, old.last_plan())
    old.close()
    _same(got, exp, what)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_matrices_on_the_admission_boundary_give_the_int64_model_s_codes(layout):
    """The largest coefficients crtfx_field420_create admits — one entry carrying the whole sum, and the sum spread over a row with both
    signs — under offsets at either end of their range: the kernels' int32 sums (8-bit: the accumulator; 10-bit: the header's
    rearrangement) and their 24-bit multiplies give the codes of the int64 model, on both paths and under every chroma value."""
    import torch
    from pythoncrt_amd import tables
    lib = _lib.load()
    deep = layout in model.DEEP
    s = (2 ** 31 - 2 ** 15 - 1) // 1024 if deep else (2 ** 31 - 2 ** 20 - 1) // 8160
    top = 1023 if deep else 255
    h, w = 10, 24
    packed = _images((h, w), layout)
    src = torch.from_numpy(packed).to(_dev())
    cases = [(np.array([[s, 0, 0], [0, -s, 0], [0, 0, s]]), (0, top, 0)),
             (np.array([[s - 7, -3, 4], [-5, s - 5, 0], [0, -(s // 2), -(s - s // 2)]]), (top, 0, top)),
             (np.array([[-(s // 3), s // 3, s // 3], [s // 2, s // 2, 0], [-s, 0, 0]]), (top // 4, top // 2, top // 2))]
    for m, off in cases:
        mi, oi = np.ascontiguousarray(m.reshape(-1), dtype=np.int32), np.ascontiguousarray(off, dtype=np.int32)
        plan = ctypes.c_void_p()
        assert lib.crtfx_field420_create(_dev().index, h, w, _lib.PIX_F16 if deep else _lib.PIX_U8, model.LAYOUTS.index(layout), tables.ptr(mi), tables.ptr(oi),
                                         ctypes.byref(plan)) == _lib.OK, lib.crtfx_field420_last_error(None)
        for chroma in CHROMAS:
            exp = np.stack([model.unpack(p, h, w, layout, chroma, m=m, off=off) for p in packed])
            for force in (0, 1):
                assert lib.crtfx_field420_set_option(plan, _lib.FIELD420_OPT_CHROMA, CHROMAS.index(chroma)) == _lib.OK
                assert lib.crtfx_field420_set_option(plan, _lib.FIELD420_OPT_FORCE_GENERAL, force) == _lib.OK
                dst = torch.empty((3, h, w, 3), dtype=torch.float16 if deep else torch.uint8, device=_dev())
                assert lib.crtfx_field420_run(plan, src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0) * dst.element_size(), 3,
                                              torch.cuda.current_stream().cuda_stream) == _lib.OK
                torch.cuda.synchronize()
                buf = ctypes.create_string_buffer(128)
                assert lib.crtfx_field420_last_plan(plan, buf, 128) == _lib.OK
                assert buf.value.decode() == _name(layout, not force, chroma, 3), buf.value
                _same(dst.cpu().numpy(), exp, (buf.value.decode(), off))
        assert lib.crtfx_field420_destroy(plan) == _lib.OK


# ---- the chroma option on a live plan ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
def test_switching_the_chroma_on_a_live_plan(layout):
    """set_option(CHROMA) back and forth on one plan, on both paths: each run gives the bytes of the model at that chroma."""
    import torch
    from pythoncrt_amd import UnpackField420
    from pythoncrt_amd._lib import CrtfxError
    size = (10, 24)
    src = torch.from_numpy(_images(size, layout)).to(_dev())
    plan = UnpackField420(_dev(), size, layout)
    assert plan.chroma == "replicate" and plan.last_plan() == _name(layout, True, "replicate", 0) and plan.plan()["chroma"] == "replicate"
    for chroma, force in (("center", False), ("left", False), ("replicate", True), ("center", True), ("center", False), ("replicate", False), ("left", True)):
        plan.chroma = chroma
        plan.force_general = force
        assert plan.chroma == chroma and plan.last_plan() == _name(layout, not force, chroma, 0)
        got = plan(src).cpu().numpy()
        how = plan.last_plan()
        assert how == _name(layout, not force, chroma, 3), how
        _same(got, _expected(size, layout, chroma), how)
    plan.set_option(_lib.FIELD420_OPT_CHROMA, _lib.FIELD420_CENTER)
    assert plan.chroma == "center"
    for option, value, word in ((_lib.FIELD420_OPT_CHROMA, 3, "CHROMA"), (_lib.FIELD420_OPT_CHROMA, -1, "CHROMA"), (_lib.FIELD420_OPT_FORCE_GENERAL, 2, "FORCE_GENERAL"),
                                (3, 0, "option"), (0, 1, "option")):
        with pytest.raises(CrtfxError) as e:
            plan.set_option(option, value)
        assert e.value.code == _lib.E_INVALID and word in str(e.value)
    assert plan.chroma == "center" and plan.last_plan() == _name(layout, False, "center", 0)     # a refused option changes nothing
    with pytest.raises(ValueError):
        plan.chroma = "top-left"
    plan.close()


# ---- misaligned bases and strided batches ---------------------------------------------------------------------------------------------------

# (source offset, destination offset, source gap, destination gap, vec?): every byte offset of a base inside a dword, unequal strides
STRIDES8 = [(0, 0, 8, 12, True), (4, 8, 4, 4, True), (1, 0, 4, 4, False), (2, 0, 4, 4, False), (3, 0, 4, 4, False), (0, 1, 4, 4, False),
            (0, 2, 4, 4, False), (0, 3, 4, 4, False), (0, 0, 3, 4, False), (0, 0, 4, 5, False), (0, 0, 2, 4, False), (3, 1, 1, 7, False)]
STRIDES10 = [(0, 0, 8, 12, True), (4, 8, 4, 4, True), (2, 0, 4, 4, False), (0, 2, 4, 4, False), (0, 0, 2, 4, False), (0, 0, 4, 6, False), (2, 6, 2, 2, False)]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_offset_and_strided_batches_leave_the_gaps_alone(layout):
    """n = 3 frames of 18 x 40 that are slices of bigger sentinel-filled buffers on both sides, chroma left.  A base that is no multiple
    of 4, or a stride that is none, takes general; multiples of 4 stay on vec.  Every frame right, every sentinel byte outside the frames
    untouched.  A 10-bit layout refuses an odd base or stride and writes nothing."""
    import torch
    from pythoncrt_amd import UnpackField420
    size, n = (18, 40), 3
    deep = layout in model.DEEP
    src = _images(size, layout)
    exp = _expected(size, layout, "left")
    sbytes, dbytes = src.shape[1], size[0] * size[1] * (6 if deep else 3)
    plan = UnpackField420(_dev(), size, layout, chroma="left")
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
        assert how == _name(layout, vec, "left", 3), (how, s_off, d_off, s_pad, d_pad)
        _same(out.cpu().numpy(), exp, (how, s_off, d_off, s_pad, d_pad))
        keep = torch.ones_like(dbuf, dtype=torch.bool)
        keep[d_off:d_off + n * (dbytes + d_pad)].view(n, dbytes + d_pad)[:, :dbytes] = False
        assert bool((dbuf[keep] == 0x5A).all()), (how, s_off, d_off)
    if deep:
        sbuf = torch.zeros((n * sbytes + 16,), dtype=torch.uint8, device=_dev())
        dbuf = torch.full((n * dbytes + 16,), 0x5A, dtype=torch.uint8, device=_dev())
        run, err, st = plan.lib.crtfx_field420_run, plan.lib.crtfx_field420_last_error, torch.cuda.current_stream().cuda_stream
        sp, dp = sbuf.data_ptr(), dbuf.data_ptr()
        for args in ((sp + 1, sbytes, dp, dbytes), (sp, sbytes, dp + 1, dbytes), (sp, sbytes + 1, dp, dbytes), (sp, sbytes, dp, dbytes + 1)):
            assert run(plan._plan, args[0], args[1], args[2], args[3], 2, st) == _lib.E_INVALID and b"odd" in err(plan._plan), (plan.last_plan(), args)
        torch.cuda.synchronize()
        assert bool((dbuf == 0x5A).all()), plan.last_plan()
    assert tuple(plan.planes(sview)[0].shape) == (n,) + size
    plan.close()


# ---- batch sizes, refusals, plan strings ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["nv12", "yuv420p10le"])
def test_an_empty_batch_and_a_batch_of_65(layout):
    """n = 0 launches nothing and leaves the plan string; 65 frames of 6 x 8 (the three test frames, repeated) are one grid on either path."""
    import torch
    from pythoncrt_amd import UnpackField420
    size = (6, 8)
    plan = UnpackField420(_dev(), size, layout, chroma="center")
    out = plan(torch.empty((0, plan.frame_bytes), dtype=torch.uint8, device=_dev()))
    assert tuple(out.shape) == (0,) + size + (3,) and plan.last_plan() == _name(layout, True, "center", 0)
    pick = np.arange(65) % 3
    src = torch.from_numpy(_images(size, layout)[pick]).to(_dev())
    for force in (False, True):
        plan.force_general = force
        got = plan(src).cpu().numpy()
        how = plan.last_plan()
        assert how == _name(layout, not force, "center", 65), how
        _same(got, _expected(size, layout, "center")[pick], how)
    plan.close()


def test_run_refuses_what_it_cannot_do():
    import torch
    from pythoncrt_amd import UnpackField420
    from pythoncrt_amd._lib import CrtfxError
    size = (8, 16)
    plan = UnpackField420(_dev(), size, "nv12")
    fb, st = plan.frame_bytes, torch.cuda.current_stream().cuda_stream
    src = torch.zeros((2, fb), dtype=torch.uint8, device=_dev())
    dst = torch.full((2,) + size + (3,), 0x5A, dtype=torch.uint8, device=_dev())
    run, err = plan.lib.crtfx_field420_run, plan.lib.crtfx_field420_last_error
    rgb = size[0] * size[1] * 3
    for args, word in (((None, fb, dst.data_ptr(), rgb, 2), "null"), ((src.data_ptr(), fb, None, rgb, 2), "null"), ((src.data_ptr(), fb, dst.data_ptr(), rgb, 0), "n = 0"),
                       ((src.data_ptr(), fb, dst.data_ptr(), rgb, -1), "n = -1"), ((src.data_ptr(), fb - 1, dst.data_ptr(), rgb, 2), "strides"),
                       ((src.data_ptr(), fb, dst.data_ptr(), rgb - 1, 2), "strides")):
        assert run(plan._plan, *args, st) == _lib.E_INVALID and word.encode() in err(plan._plan), (args, err(plan._plan))
    torch.cuda.synchronize()
    assert bool((dst == 0x5A).all()) and plan.last_plan() == _name("nv12", True, "replicate", 0)
    with pytest.raises(CrtfxError) as e:
        plan(src.view(torch.int8))
    assert e.value.code == _lib.E_UNSUPPORTED
    for bad in (src[:, :-1], src.cpu()):
        with pytest.raises(ValueError):
            plan(bad)
    with pytest.raises(ValueError):
        plan(src, out=dst[:1])
    plan.close()
    for size, word in (((7, 16), "odd"), ((2, 16), "below 4")):
        with pytest.raises(CrtfxError) as e:
            UnpackField420(_dev(), size, "nv12")
        assert e.value.code == _lib.E_INVALID and word in str(e.value)


def test_last_plan_strings():
    from pythoncrt_amd import UnpackField420
    for layout in LAYOUTS:
        for size, vec in (((8, 16), True), ((8, 12), False), ((6, 1), False)):
            plan = UnpackField420(_dev(), size, layout, chroma="left")
            assert plan.last_plan() == _name(layout, vec, "left", 0) and plan.plan() == {"field420": f"k_unpack_field420<{layout},{'vec' if vec else 'general'}>", "chroma": "left", "frames": "0"}
            plan.force_general = True
            assert plan.last_plan() == _name(layout, False, "left", 0)
            plan.close()
    lib = _lib.load()
    buf = ctypes.create_string_buffer(8)
    assert lib.crtfx_field420_last_plan(None, buf, 8) == _lib.E_INVALID


# ---- whole frames -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size,n", [((480, 720), 2), ((1080, 1920), 1)], ids=["480i", "1080i"])
@pytest.mark.parametrize("layout,chroma", [("nv12", "left"), ("p010le", "left"), ("yuv420p", "replicate")])
def test_one_batch_of_whole_frames(layout, chroma, size, n):
    """Random frames of 480 x 720 and 1080 x 1920 per sample type, on the vec path."""
    fb = model.frame_bytes(size[0], size[1], layout)
    rs = np.random.default_rng(size[0])
    if layout in model.DEEP:
        packed = deep_model.to_bytes(rs.integers(0, 1024, (n, fb // 2)).astype(np.uint16) << 6).reshape(n, fb)
    else:
        packed = rs.integers(0, 256, (n, fb), dtype=np.uint8)
    got, how = _run(packed, size, layout, chroma)
    assert how == _name(layout, True, chroma, n), how
    for i in range(n):
        _same(got[i], model.unpack(packed[i], size[0], size[1], layout, chroma), (how, i))
