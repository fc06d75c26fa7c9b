"""The field-paired 4:2:0 egress stage on the GPU: EgressField420 (k_egress_field420, four layouts x vec / general, chroma center / left)
against the int64 host model of tests/egress_field420_model.py — equality is zero differing elements, and every assert names the plan
string — and against the existing box plans run on the two fields on the device ("center" is their weave)."""
import functools

import numpy as np
import pytest

from pythoncrt_amd import _lib
from tests import deep_model
from tests import egress_field420_model as model

pytestmark = pytest.mark.gpu

SIZES = [(4, 1), (4, 8), (8, 7), (8, 16), (12, 24), (16, 136), (20, 9), (24, 40)]
LAYOUTS = list(model.LAYOUTS)
CHROMAS = list(model.CHROMAS)
ids = dict(ids=lambda s: f"{s[0]}x{s[1]}")


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _name(layout, vec, chroma, frames):
    return f"egress_field420=k_egress_field420<{layout},{'vec' if vec else 'general'}>;chroma={chroma};frames={frames}"


def _plan(size, layout, chroma="center", force_general=False, matrix="bt601", rng="tv"):
    from pythoncrt_amd import EgressField420
    plan = EgressField420(_dev(), size, layout, matrix=matrix, range=rng, chroma=chroma, force_general=force_general)
    assert plan.chroma == chroma and plan.force_general == force_general and plan.frame_bytes == model.frame_bytes(size[0], size[1], layout)
    return plan


def _run(frames_np, layout, chroma="center", force_general=False, matrix="bt601", rng="tv"):
    """(uint8 [n, frame_bytes] from the device, last_plan) for a stack of RGB frames."""
    import torch
    plan = _plan(tuple(frames_np.shape[1:3]), layout, chroma, force_general, matrix, rng)
    out = plan(torch.from_numpy(frames_np).to(_dev()))
    torch.cuda.synchronize()
    got, how = out.cpu().numpy(), plan.last_plan()
    assert got.dtype == np.uint8 and got.shape == (frames_np.shape[0], plan.frame_bytes)
    plan.close()
    return got, how


@functools.lru_cache(maxsize=None)
def _images(size, deep):
    """uint8 random / binary / clamp-colour frames, or half frames over the quarter codes: the existing family models' three."""
    return model.images(size[0], size[1], "p010le" if deep else "nv12")


@functools.lru_cache(maxsize=None)
def _expected(size, layout, chroma, matrix="bt601", rng="tv"):
    """The model's frames of _images(size, .): computed once, shared, never written to."""
    exp = model.pack_batch(_images(size, layout in model.DEEP), layout, chroma, matrix, rng)
    exp.flags.writeable = False
    return exp


def _same(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape)
    bad = int((got != exp).sum())
    assert bad == 0, (what, bad)


# ---- frames equal the model ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("force_general", [False, True], ids=["default", "general"])
@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", SIZES, **ids)
def test_frames_equal_the_model(size, layout, chroma, force_general):
    """Batches of 1, 2 and 3 frames of: 4 x 1, every tap clamped both ways; 4 x 8, one vec lane per lane row and all four vertical taps
    clamped; 8 x 7 and 20 x 9, odd widths; 8 x 16, first and last field chroma rows adjacent; 12 x 24, a field chroma row with no clamped
    tap, three lanes per row (the left-neighbour load across lanes and at a row start); 16 x 136, 17 lanes per row so that lane rows straddle
    waves and a second block; 24 x 40.  The plan says vec exactly where w % 8 == 0 and nothing is forced, and always names the chroma."""
    import torch
    deep = layout in model.DEEP
    src = torch.from_numpy(np.asarray(_images(size, deep))).to(_dev())
    plan = _plan(size, layout, chroma, force_general)
    exp = _expected(size, layout, chroma)
    for n in (1, 2, 3):
        got = plan(src[3 - n:]).cpu().numpy()
        how = plan.last_plan()
        assert how == _name(layout, size[1] % 8 == 0 and not force_general, chroma, n), how
        _same(got, exp[3 - n:], (size, how))
    plan.close()


@pytest.mark.parametrize("force_general", [False, True], ids=["default", "general"])
@pytest.mark.parametrize("matrix,rng", model.CASES)
@pytest.mark.parametrize("size", [(20, 9), (12, 24)], **ids)
def test_every_matrix_and_range(size, matrix, rng, force_general):
    for layout in LAYOUTS:
        for chroma in CHROMAS:
            got, how = _run(np.asarray(_images(size, layout in model.DEEP)), layout, chroma, force_general, matrix=matrix, rng=rng)
            assert how == _name(layout, size[1] % 8 == 0 and not force_general, chroma, 3), how
            _same(got, _expected(size, layout, chroma, matrix, rng), (size, matrix, rng, how))


def _run_matrix(frames_np, layout, chroma, force_general, m, off):
    """A run with a matrix of the test's own through the C ABI: EgressField420's tables replaced for one construction."""
    import torch
    from pythoncrt_amd import EgressField420

    class Custom(EgressField420):
        def _tables(self):
            return np.ascontiguousarray(np.asarray(m).reshape(-1), dtype=np.int32), np.ascontiguousarray(off, dtype=np.int32)
    plan = Custom(_dev(), tuple(frames_np.shape[1:3]), layout, chroma=chroma, force_general=force_general)
    got, how = plan(torch.from_numpy(frames_np).to(_dev())).cpu().numpy(), plan.last_plan()
    plan.close()
    return got, how


@pytest.mark.parametrize("force_general", [False, True], ids=["vec", "general"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_matrix_on_the_admission_boundary(layout, force_general):
    """The U row with the largest sums create admits (tests/egress_field420_model.boundary_matrix), on the frames that drive it to both
    ends and on the three test frames: the accumulator ends within one X of 2^31 (8-bit) or 2^32 (10-bit) and of 0.  One step past the
    boundary create refuses."""
    from pythoncrt_amd._lib import CrtfxError
    size = (8, 16)
    inside, outside = model.boundary_matrix(layout)
    off = model.tables(layout)[1]
    top_code = 1020 if layout in model.DEEP else 255
    ends = np.stack([model.to_frame(np.broadcast_to(np.array(c), size + (3,)), layout) for c in ((top_code, 0, top_code), (0, top_code, 0))])
    frames = np.concatenate([ends, np.asarray(_images(size, layout in model.DEEP))])
    for chroma in CHROMAS:
        got, how = _run_matrix(frames, layout, chroma, force_general, inside, off)
        assert how == _name(layout, not force_general, chroma, 5), how
        _same(got, model.pack_batch(frames, layout, chroma, m=inside, off=off), how)
    with pytest.raises(CrtfxError) as e:
        _run_matrix(frames, layout, "center", force_general, outside, off)
    assert e.value.code == _lib.E_INVALID and "accumulator" in str(e.value)


@pytest.mark.parametrize("force_general", [False, True], ids=["vec", "general"])
@pytest.mark.parametrize("size", [(4, 8), (8, 16)], **ids)
@pytest.mark.parametrize("layout", model.DEEP)
def test_the_10_bit_frames_that_drive_an_accumulator_to_its_maximum(layout, size, force_general):
    """1020 in the channels with positive entries of the U / V row and 0 in the others (and the reverse): accumulators above 2^31 — up to
    1.99999 * 2^31 in full range — in every chroma sample, for every matrix and both chroma values."""
    for matrix, rng in model.CASES:
        frames = np.stack([model.extreme_frame(size[0], size[1], layout, row, matrix, rng, low) for row in (1, 2) for low in (False, True)])
        acc = model.accumulators(model.pixel_codes(frames[0], layout), layout, "left", matrix, rng)[1]
        assert acc.min() > 2 ** 31
        for chroma in CHROMAS:
            got, how = _run(frames, layout, chroma, force_general, matrix=matrix, rng=rng)
            assert how == _name(layout, not force_general, chroma, 4), how
            _same(got, model.pack_batch(frames, layout, chroma, matrix, rng), (matrix, rng, how))


# ---- 10-bit: the quantiser and the bits outside a sample ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("force_general", [False, True], ids=["vec", "general"])
@pytest.mark.parametrize("layout", model.DEEP)
def test_every_half_bit_pattern_and_the_bits_outside_a_sample(layout, force_general):
    """144 x 160 x 3 = 69 120 samples in one frame: sample i of the flat half array has pattern i mod 65536 — NaNs of both kinds,
    infinities, negatives, -0, subnormals and every tie of the quantiser; a second frame has them in reversed order (so the filter mixes
    them otherwise).  Equal to the model bit for bit at both chroma values, and the six bits of every word outside its sample are 0."""
    h, w = 144, 160
    pat = (np.arange(h * w * 3, dtype=np.int64) % 65536).astype(np.uint16)
    frames = np.stack([pat, pat[::-1]]).view(np.float16).reshape(2, h, w, 3)
    assert len(set(frames[0].view(np.uint16).reshape(-1).tolist())) == 65536
    for chroma in CHROMAS:
        got, how = _run(frames, layout, chroma, force_general)
        assert how == _name(layout, not force_general, chroma, 2), how
        _same(got, model.pack_batch(frames, layout, chroma), how)
        words = deep_model.words(got)
        assert int((words & (0x003F if layout == "p010le" else 0xFC00)).sum()) == 0, how


# ---- "center" against the existing box plans on the two fields -----------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", [(8, 7), (12, 24), (16, 136)], **ids)
def test_center_is_the_weave_of_the_box_plans_on_the_two_fields_on_the_device(size, layout):
    """The three frames' fields, copied contiguous, through the EXISTING box plan of the layout at h/2 x w on the device; the planes woven
    on the host: "center" gives those bytes on both paths, and "left" does not (Y always does)."""
    import torch
    from pythoncrt_amd import formats
    h, w = size
    frames = np.asarray(_images(size, layout in model.DEEP))
    src = torch.from_numpy(frames).to(_dev())
    old = formats.FORMATS[layout].egress(_dev(), (h // 2, w), layout=layout)
    fields = [old(src[:, f::2].contiguous()).cpu().numpy() for f in (0, 1)]
    old_how = old.last_plan()
    old.close()
    ref = []
    for i in range(3):
        parts = [model.samples(fields[f][i], h // 2, w, layout) for f in (0, 1)]
        y, u, v = (np.empty((n,) + parts[0][k].shape[1:], dtype=np.int64) for k, n in ((0, h), (1, h // 2), (2, h // 2)))
        for f in (0, 1):
            y[f::2], u[f::2], v[f::2] = parts[f]
        ref.append(model.write(y, u, v, layout))
    ref = np.stack(ref)
    for force in (False, True):
        got, how = _run(frames, layout, "center", force)
        _same(got, ref, (size, how, old_how))
    left, how = _run(frames, layout, "left")
    a, b = model.samples(left[0], h, w, layout), model.samples(ref[0], h, w, layout)
    assert np.array_equal(a[0], b[0]), (how, old_how)
    differ = np.concatenate([(a[k] != b[k]).reshape(-1) for k in (1, 2)])
    print(how, old_how, "chroma samples that differ", float(differ.mean()))
    assert differ.mean() >= 0.5, (how, old_how, float(differ.mean()))


# ---- the chroma option on a live plan ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
def test_switching_the_chroma_on_a_live_plan(layout):
    """set_option(CHROMA) back and forth on one plan, on both paths: each run gives the bytes of the model of that chroma value."""
    import torch
    from pythoncrt_amd import EgressField420
    from pythoncrt_amd._lib import CrtfxError
    size = (12, 24)
    deep = layout in model.DEEP
    src = torch.from_numpy(np.asarray(_images(size, deep))).to(_dev())
    plan = EgressField420(_dev(), size, layout)
    assert plan.chroma == "center" and plan.last_plan() == _name(layout, True, "center", 0) and plan.plan()["chroma"] == "center"
    for chroma, force in (("left", False), ("center", False), ("left", True), ("left", False), ("center", True), ("center", False)):
        plan.chroma = chroma
        plan.force_general = force
        assert plan.chroma == chroma and plan.last_plan() == _name(layout, not force, chroma, 0)
        got = plan(src).cpu().numpy()
        how = plan.last_plan()
        assert how == _name(layout, not force, chroma, 3), how
        _same(got, _expected(size, layout, chroma), how)
    plan.set_option(_lib.EGRESS_FIELD420_OPT_CHROMA, _lib.EGRESS_FIELD420_LEFT)
    assert plan.chroma == "left"
    for option, value, word in ((_lib.EGRESS_FIELD420_OPT_CHROMA, 2, "CHROMA"), (_lib.EGRESS_FIELD420_OPT_CHROMA, -1, "CHROMA"),
                                (_lib.EGRESS_FIELD420_OPT_FORCE_GENERAL, 2, "FORCE_GENERAL"), (3, 0, "option"), (0, 1, "option")):
        with pytest.raises(CrtfxError) as e:
            plan.set_option(option, value)
        assert e.value.code == _lib.E_INVALID and word in str(e.value)
    assert plan.chroma == "left" and plan.last_plan() == _name(layout, True, "left", 0)         # a refused option changes nothing
    with pytest.raises(ValueError):
        plan.chroma = "replicate"
    plan.close()


# ---- misaligned bases and strided batches ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_byte_offset_inside_guarded_tensors_with_unequal_strides(layout):
    """n = 3 frames of 12 x 24 that are slices of bigger sentinel-filled buffers on both sides, chroma left, at every base offset 0..3 on
    either side and frame gaps that differ between the sides (10-bit: the even ones).  A base that is no multiple of 4, or a stride that is
    none, takes general; multiples of 4 stay on vec.  Every frame right, every guard byte outside the frames untouched.  A 10-bit layout
    refuses an odd base or stride and writes nothing."""
    import torch
    size, n = (12, 24), 3
    deep = layout in model.DEEP
    src = np.asarray(_images(size, deep))
    exp = _expected(size, layout, "left")
    sbytes, dbytes = size[0] * size[1] * (6 if deep else 3), exp.shape[1]
    assert sbytes % 4 == 0 and dbytes % 4 == 0
    step = 2 if deep else 1
    cases = [(s, d, sp, dp) for s in range(0, 4, step) for d in range(0, 4, step) for sp, dp in ((4, 8), (8 - step, 4), (4, 12 + step))]
    plan = _plan(size, layout, "left")
    seen = set()
    for s_off, d_off, s_pad, d_pad in cases:
        vec = not ((s_off | d_off | s_pad | d_pad) & 3)
        sbuf = torch.full((s_off + n * (sbytes + s_pad) + 16,), 0xEE, dtype=torch.uint8, device=_dev())
        dbuf = torch.full((d_off + n * (dbytes + d_pad) + 16,), 0x5A, dtype=torch.uint8, device=_dev())
        assert sbuf.data_ptr() % 4 == 0 and dbuf.data_ptr() % 4 == 0
        sview = sbuf[s_off:s_off + n * (sbytes + s_pad)].view(n, sbytes + s_pad)[:, :sbytes]
        dview = dbuf[d_off:d_off + n * (dbytes + d_pad)].view(n, dbytes + d_pad)[:, :dbytes]
        sview.copy_(torch.from_numpy(np.ascontiguousarray(src).view(np.uint8).reshape(n, sbytes)).to(_dev()))
        if deep:                                                    # a half view of bytes at an even offset, through the C ABI's pointers
            rc = plan.lib.crtfx_egress_field420_run(plan._plan, sview.data_ptr(), sbytes + s_pad, dview.data_ptr(), dbytes + d_pad, n, torch.cuda.current_stream().cuda_stream)
            assert rc == _lib.OK, plan.lib.crtfx_egress_field420_last_error(plan._plan)
        else:
            assert plan(sview.unflatten(1, size + (3,)), out=dview) is dview
        torch.cuda.synchronize()
        how = plan.last_plan()
        assert how == _name(layout, vec, "left", 3), (how, s_off, d_off, s_pad, d_pad)
        _same(dview.cpu().numpy(), exp, (how, s_off, d_off, s_pad, d_pad))
        keep = torch.ones_like(dbuf, dtype=torch.bool)
        keep[d_off:d_off + n * (dbytes + d_pad)].view(n, dbytes + d_pad)[:, :dbytes] = False
        assert bool((dbuf[keep] == 0x5A).all()), (how, s_off, d_off)
        seen.add(vec)
    assert seen == {True, False}
    if deep:
        sbuf = torch.zeros((n * sbytes + 16,), dtype=torch.uint8, device=_dev())
        dbuf = torch.full((n * dbytes + 16,), 0x5A, dtype=torch.uint8, device=_dev())
        run, err, st = plan.lib.crtfx_egress_field420_run, plan.lib.crtfx_egress_field420_last_error, torch.cuda.current_stream().cuda_stream
        sp, dp = sbuf.data_ptr(), dbuf.data_ptr()
        for args in ((sp + 1, sbytes, dp, dbytes), (sp, sbytes, dp + 1, dbytes), (sp, sbytes + 1, dp, dbytes), (sp, sbytes, dp, dbytes + 1), (sp + 3, sbytes, dp + 3, dbytes)):
            assert run(plan._plan, args[0], args[1], args[2], args[3], 2, st) == _lib.E_INVALID and b"odd" in err(plan._plan), (plan.last_plan(), args)
        torch.cuda.synchronize()
        assert bool((dbuf == 0x5A).all()), plan.last_plan()
    assert tuple(plan.planes(dview)[0].shape) == (n,) + size
    plan.close()


# ---- n = 0, a long batch, the refusals of run, the plan strings -------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
def test_empty_and_long_batches_refusals_of_run_and_plan_strings(layout):
    import torch
    from pythoncrt_amd._lib import CrtfxError
    size = (8, 16)
    deep = layout in model.DEEP
    imgs = np.asarray(_images(size, deep))
    exp = _expected(size, layout, "center")
    plan = _plan(size, layout)
    assert plan.last_plan() == _name(layout, True, "center", 0) and plan.plan() == {"egress_field420": f"k_egress_field420<{layout},vec>", "chroma": "center", "frames": "0"}
    rgb = torch.float16 if deep else torch.uint8
    empty = plan(torch.empty((0,) + size + (3,), dtype=rgb, device=_dev()))
    assert tuple(empty.shape) == (0, plan.frame_bytes) and plan.last_plan() == _name(layout, True, "center", 0)
    pick = np.arange(65) % 3
    got = plan(torch.from_numpy(imgs[pick]).to(_dev())).cpu().numpy()
    assert plan.last_plan() == _name(layout, True, "center", 65)
    _same(got, exp[pick], plan.last_plan())
    plan.force_general = True
    assert plan.last_plan() == _name(layout, False, "center", 0)
    # the refusals of run
    src = torch.from_numpy(imgs).to(_dev())
    with pytest.raises(CrtfxError) as e:                            # the other pixel format
        plan(torch.zeros((1,) + size + (3,), dtype=torch.uint8 if deep else torch.float16, device=_dev()))
    assert e.value.code == _lib.E_UNSUPPORTED
    for bad in (src[:, :4], src[:, :, :8], src.cpu()):
        with pytest.raises(ValueError):
            plan(bad)
    with pytest.raises(ValueError):
        plan(src, out=torch.empty((3, plan.frame_bytes + 1), dtype=torch.uint8, device=_dev()))
    with pytest.raises(ValueError):
        plan(src.transpose(1, 2).contiguous().transpose(1, 2))     # frames that are not contiguous
    run, err, st = plan.lib.crtfx_egress_field420_run, plan.lib.crtfx_egress_field420_last_error, torch.cuda.current_stream().cuda_stream
    out = torch.full((3, plan.frame_bytes), 0x5A, dtype=torch.uint8, device=_dev())
    sb, db = src[0].numel() * src.element_size(), plan.frame_bytes
    for args, word in (((None, sb, out.data_ptr(), db, 1), b"null"), ((src.data_ptr(), sb, None, db, 1), b"null"), ((src.data_ptr(), sb, out.data_ptr(), db, 0), b"n = 0"),
                       ((src.data_ptr(), sb, out.data_ptr(), db, -1), b"n = -1"), ((src.data_ptr(), sb - 4, out.data_ptr(), db, 2), b"smaller than a frame"),
                       ((src.data_ptr(), sb, out.data_ptr(), db - 4, 2), b"smaller than a frame")):
        assert run(plan._plan, *args, st) == _lib.E_INVALID and word in err(plan._plan), (args, err(plan._plan))
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())
    with pytest.raises(CrtfxError) as e:
        _plan((6, 16), layout)
    assert e.value.code == _lib.E_INVALID and "multiple of 4" in str(e.value)
    plan.close()


# ---- full-size batches ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["nv12", "p010le"])
@pytest.mark.parametrize("size", [(480, 720), (1080, 1920)], **ids)
def test_one_full_size_batch(size, layout):
    """2 frames of 480 x 720 and of 1080 x 1920 per sample type, on the vec path, chroma left."""
    rs = np.random.default_rng(size[0])
    if layout in model.DEEP:
        frames = (rs.integers(0, 2048, (2,) + size + (3,)) / 8.0).astype(np.float16)       # eighths: ties of the quantiser among them
    else:
        frames = rs.integers(0, 256, (2,) + size + (3,), dtype=np.uint8)
    got, how = _run(frames, layout, "left")
    assert how == _name(layout, True, "left", 2), how
    for i in range(2):
        _same(got[i], model.pack(frames[i], layout, "left"), (how, i))
