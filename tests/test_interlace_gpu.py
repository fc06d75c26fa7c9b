"""The interlace stage on the GPU (include/crtfx_interlace.h) against tests/interlace_model.py: both sample types, both orders, the three
low-pass settings, both paths.  Every comparison is exact: no element may differ."""
import itertools

import numpy as np
import pytest

from pythoncrt_amd import _lib
from tests import deint_model
from tests import interlace_model as model

pytestmark = pytest.mark.gpu

GUARD = 0xA5
# h = 2, 3, 4: every clamped row index; w = 1, 3, 5: no vec block; 8: one; 16, 24, 40: several; 33: several lanes and a width that is no
# multiple of 8; 16 x 8 and 23 x 40: an even and an odd height over more than one wave
SHAPES = [(2, 1), (2, 8), (3, 5), (4, 16), (5, 8), (6, 3), (7, 24), (16, 8), (9, 33), (23, 40)]
COUNTS = (1, 2, 3, 5, 8)
DTYPES = {"u8": np.uint8, "f16": np.float16}
COMBOS = list(itertools.product(model.ORDERS, model.LOWPASS))


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _torch_dtype(pix):
    import torch
    return torch.uint8 if pix == "u8" else torch.float16


def _plan(size, pix, order, lowpass, force=False):
    import pythoncrt_amd as pc
    return pc.Interlace(_dev(), size, order=order, lowpass=lowpass, dtype=_torch_dtype(pix), force_general=force)


def _source(pix, shape, seed):
    """Noise: bytes; or halves that cross every rule — quarter codes, values between them and past both ends, NaN, infinities, -0."""
    rng = np.random.default_rng(seed)
    if pix == "u8":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    f = (rng.integers(-40, 8 * 1030, shape) / 32.0).astype(np.float16)
    flat = f.reshape(-1)
    pick = rng.integers(0, flat.size, max(1, flat.size // 16))
    flat[pick] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0, 255.5, 254.875, 0.125, 6e-8, 65504.0], dtype=np.float16), pick.size)
    return f


def _same(got, exp):
    """Bit for bit: halves are compared as their patterns."""
    assert got.dtype == exp.dtype and got.shape == exp.shape, (got.dtype, exp.dtype, got.shape, exp.shape)
    return int((model.bits(got) != model.bits(exp)).sum())


def _vec_expected(w, src, dst, n, force=False):
    """The header's conditions, from the tensors' own addresses and strides."""
    if force or w % 8 or (src.data_ptr() | dst.data_ptr()) & 3:
        return False
    if n > 1 and (src.stride(0) * src.element_size()) & 3:
        return False
    return n <= 2 or not (dst.stride(0) * dst.element_size()) & 3


def _name(lowpass, pix, vec):
    return f"k_interlace<{lowpass},{pix},{'vec' if vec else 'general'}>"


@pytest.mark.parametrize("force", [False, True], ids=["auto", "forced"])
@pytest.mark.parametrize("pix", list(DTYPES))
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_and_frame_counts_against_the_model(size, pix, force):
    import torch
    src = _source(pix, (max(COUNTS),) + size + (3,), [size[0], size[1]])
    x = torch.from_numpy(src).to(_dev())
    for order, lowpass in COMBOS:
        plan = _plan(size, pix, order, lowpass, force)
        assert plan.frames_in == 2 and plan.frames_out == 1
        for n in COUNTS:
            out = plan.run(x[:n])
            torch.cuda.synchronize()
            assert tuple(out.shape) == ((n + 1) // 2,) + size + (3,)
            assert _same(out.cpu().numpy(), model.interlace(src[:n], order, lowpass)) == 0, (size, pix, order, lowpass, force, n)
            vec = _vec_expected(size[1], x[:n], out, n, force)
            assert plan.plan() == {"interlace": _name(lowpass, pix, vec), "frames": str(n)}, plan.last_plan()
            if not force:                                                      # fresh allocations are aligned: the vec path wherever the width lets it
                assert vec == (size[1] % 8 == 0)
        plan.close()


@pytest.mark.parametrize("force", [False, True], ids=["vec", "general"])
def test_every_half_pattern_kept_and_filtered(force):
    """All 65 536 half patterns in each of the five rows of two 5 x 21848 frames, rolled differently: NONE keeps every pattern's bits in the
    row of the frame the order names; under LINEAR and COMPLEX every pattern is r(0) and a neighbour of every tap."""
    import torch
    w = 21848                                                                   # 8 * 2731 pixels: 65 544 samples per row
    pats = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    src = np.stack([np.stack([np.concatenate([np.roll(pats, 7919 * (5 * f + y)), pats[:8]]) for y in range(5)]) for f in range(2)])
    src = src.view(np.float16).reshape(2, 5, w, 3)
    x = torch.from_numpy(src).to(_dev())
    for order, lowpass in COMBOS:
        plan = _plan((5, w), "f16", order, lowpass, force)
        got = plan.run(x).cpu().numpy()
        assert plan.plan() == {"interlace": _name(lowpass, "f16", not force), "frames": "2"}
        assert _same(got, model.interlace(src, order, lowpass)) == 0, (order, lowpass)
        if lowpass == "none":
            first = model.ORDERS.index(order)
            assert np.array_equal(model.bits(got[0, first::2]), model.bits(src[0, first::2]))
            assert np.array_equal(model.bits(got[0, 1 - first::2]), model.bits(src[1, 1 - first::2]))
        plan.close()


def _guarded(n, frame_bytes, stride_bytes, offset, dtype):
    """(the guarded uint8 buffer, a [n, frame elements] view of `dtype` into it at byte `offset` with frame stride `stride_bytes`)."""
    import torch
    pad = 64
    total = pad + offset + (n - 1) * stride_bytes + frame_bytes + pad
    total += total & 1
    buf = torch.full((total,), GUARD, dtype=torch.uint8, device=_dev())
    item = 2 if dtype == torch.float16 else 1
    body = buf[pad + offset:pad + offset + (n - 1) * stride_bytes + frame_bytes]
    view = body.view(dtype).as_strided((n, frame_bytes // item), (stride_bytes // item, 1))
    assert view.data_ptr() == buf.data_ptr() + pad + offset
    return buf, view


def _guards_intact(buf, n, frame_bytes, stride_bytes, offset):
    b = buf.cpu().numpy().copy()
    pad = 64
    for i in range(n):
        lo = pad + offset + i * stride_bytes
        b[lo:lo + frame_bytes] = GUARD
    return bool((b == GUARD).all())


@pytest.mark.parametrize("lowpass", model.LOWPASS)
@pytest.mark.parametrize("pix", list(DTYPES))
@pytest.mark.parametrize("size", [(3, 8), (9, 24), (5, 13)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_base_offset_inside_guards(size, pix, lowpass):
    """uint8 frames at byte offsets 0..3, half frames at 0 and 2, five source frames (three written), source and destination strides that
    differ and are a few bytes longer than a frame: the bytes are the model's, the path is the one the header's conditions give, and no byte
    outside the frames changes, in the source or in the destination."""
    import torch
    h, w = size
    dt, item = _torch_dtype(pix), (1 if pix == "u8" else 2)
    fb = h * w * 3 * item
    offsets = range(4) if pix == "u8" else (0, 2)
    seen = set()
    n = 5
    n_out = 3
    plan = _plan(size, pix, "bff", lowpass)
    for s_off, d_off in itertools.product(offsets, offsets):
        for s_gap, d_gap in ((0, 4), (8, 0), (2, 6), (4, 8)) if pix == "f16" else ((0, 4), (8, 0), (3, 1), (1, 4)):
            src_np = _source(pix, (n,) + size + (3,), [h, w, s_off, d_off, s_gap])
            sb, s = _guarded(n, fb, fb + s_gap, s_off, dt)
            db, d = _guarded(n_out, fb, fb + d_gap, d_off, dt)
            s.copy_(torch.from_numpy(src_np.reshape(n, -1)).to(_dev()))
            s4 = s.as_strided((n, h, w, 3), (s.stride(0), w * 3, 3, 1))
            d4 = d.as_strided((n_out, h, w, 3), (d.stride(0), w * 3, 3, 1))
            plan.run(s4, out=d4)
            torch.cuda.synchronize()
            vec = _vec_expected(w, s4, d4, n)
            seen.add(vec)
            assert plan.plan()["interlace"] == _name(lowpass, pix, vec), (s_off, d_off, s_gap, d_gap, plan.last_plan())
            assert _same(d4.cpu().numpy(), model.interlace(src_np, "bff", lowpass)) == 0, (s_off, d_off, s_gap, d_gap)
            assert _guards_intact(db, n_out, fb, fb + d_gap, d_off) and _guards_intact(sb, n, fb, fb + s_gap, s_off)
            assert _same(s4.cpu().numpy(), src_np) == 0
    plan.close()
    assert seen == ({False} if w % 8 else {True, False})


@pytest.mark.parametrize("pix", list(DTYPES))
def test_the_strides_that_count_follow_the_frames_written(pix):
    """n = 2 writes one frame: the source stride counts, the destination's does not; n = 3 writes two: both count; n = 1: neither."""
    import torch
    size, item = (4, 8), (1 if pix == "u8" else 2)
    fb = 4 * 8 * 3 * item
    plan = _plan(size, pix, "tff", "linear")
    for n, s_gap, d_gap, vec in ((1, 2, 2, True), (2, 4, 2, True), (2, 2, 4, False), (3, 4, 4, True), (3, 4, 2, False), (3, 2, 4, False)):
        n_out = (n + 1) // 2
        src_np = _source(pix, (n,) + size + (3,), [n, s_gap, d_gap])
        sb, s = _guarded(n, fb, fb + s_gap, 0, _torch_dtype(pix))
        db, d = _guarded(n_out, fb, fb + d_gap, 0, _torch_dtype(pix))
        s.copy_(torch.from_numpy(src_np.reshape(n, -1)).to(_dev()))
        d4 = d.as_strided((n_out,) + size + (3,), (d.stride(0), 24, 3, 1))
        plan.run(s.as_strided((n,) + size + (3,), (s.stride(0), 24, 3, 1)), out=d4)
        torch.cuda.synchronize()
        assert plan.plan() == {"interlace": _name("linear", pix, vec), "frames": str(n)}, (n, s_gap, d_gap)
        assert _same(d4.cpu().numpy(), model.interlace(src_np, "tff", "linear")) == 0 and _guards_intact(db, n_out, fb, fb + d_gap, 0)
    plan.close()


@pytest.mark.parametrize("pix", list(DTYPES))
def test_batches_with_unequal_strides_and_slices(pix):
    """Slices of larger tensors: the source's batch stride and the destination's differ, and both exceed a frame."""
    import torch
    size, n = (9, 24), 5
    src_np = _source(pix, (n, 2) + size + (3,), 12)
    big_src = torch.from_numpy(src_np).to(_dev())
    big_dst = torch.zeros((3, 3) + size + (3,), dtype=_torch_dtype(pix), device=_dev())
    plan = _plan(size, pix, "tff", "complex")
    out = plan.run(big_src[:, 1], out=big_dst[:, 2])
    torch.cuda.synchronize()
    assert out.data_ptr() == big_dst[:, 2].data_ptr() and plan.plan() == {"interlace": _name("complex", pix, True), "frames": str(n)}
    assert _same(big_dst[:, 2].cpu().numpy(), model.interlace(src_np[:, 1], "tff", "complex")) == 0
    assert int(big_dst[:, :2].view(torch.uint8).sum()) == 0                     # the frames between: untouched
    with pytest.raises(ValueError, match="contiguous"):
        plan.run(torch.zeros((n,) + size + (6,), dtype=big_src.dtype, device=_dev())[..., ::2])      # the right shape, frames with holes
    plan.close()


@pytest.mark.parametrize("lowpass", model.LOWPASS)
@pytest.mark.parametrize("pix", list(DTYPES))
def test_no_frames_a_long_batch_and_the_call_forms(pix, lowpass):
    import torch
    size = (3, 8)
    plan = _plan(size, pix, "bff", lowpass)
    src_np = _source(pix, (65,) + size + (3,), 65)
    x = torch.from_numpy(src_np).to(_dev())
    out = plan.run(x)                                                          # 65 source frames of 3 x 8: 33 output frames in one grid
    torch.cuda.synchronize()
    assert plan.plan() == {"interlace": _name(lowpass, pix, True), "frames": "65"} and out.shape[0] == 33
    assert _same(out.cpu().numpy(), model.interlace(src_np, "bff", lowpass)) == 0
    assert torch.equal(plan(x).view(torch.uint8), plan.run(x).view(torch.uint8))       # plan(x) == plan.run(x)
    empty = plan.run(x[:0])
    assert tuple(empty.shape) == (0,) + size + (3,) and empty.dtype == out.dtype
    keep = out.clone()
    assert plan.run(x[:0], out=out[:0]).data_ptr() == out[:0].data_ptr()       # n = 0: `out` comes back untouched
    # n = 0 through the C entry point: nothing runs, nothing is written, nothing is asked of the pointers
    st = torch.cuda.current_stream().cuda_stream
    assert plan.lib.crtfx_interlace_run(plan._plan, x.data_ptr(), 0, out.data_ptr(), 0, 0, st) == _lib.OK
    assert plan.lib.crtfx_interlace_run(plan._plan, None, 0, None, 0, 0, st) == _lib.OK
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.uint8), keep.view(torch.uint8)) and plan.plan()["frames"] == "0"
    # force_general switches the plan string and not the bytes
    plan.force_general = True
    assert plan.force_general and plan.plan()["interlace"] == _name(lowpass, pix, False)
    forced = plan.run(x)
    torch.cuda.synchronize()
    assert plan.plan() == {"interlace": _name(lowpass, pix, False), "frames": "65"} and torch.equal(forced.view(torch.uint8), out.view(torch.uint8))
    plan.force_general = False
    assert plan.plan()["interlace"] == _name(lowpass, pix, True)
    plan.close()


@pytest.mark.parametrize("force", [False, True], ids=["vec", "general"])
@pytest.mark.parametrize("n", [32768 + 3, 32768 + 2])
def test_one_batch_across_the_launch_group_boundary(n, force):
    """The launch is grouped by grid.z, 32768 source frames (16384 output frames) per launch: a batch of 2 x 8 frames that needs a second
    launch, whose last pair is whole (n even) or an odd frame woven with itself."""
    import torch
    rng = np.random.default_rng(n)
    src = rng.integers(0, 256, (n, 2, 8, 3), dtype=np.uint8)
    plan = _plan((2, 8), "u8", "bff", "linear", force)
    out = plan.run(torch.from_numpy(src).to(_dev()))
    torch.cuda.synchronize()
    assert out.shape[0] == (n + 1) // 2 and plan.plan() == {"interlace": _name("linear", "u8", not force), "frames": str(n)}
    assert _same(out.cpu().numpy(), model.interlace(src, "bff", "linear")) == 0
    plan.close()


@pytest.mark.parametrize("pix", list(DTYPES))
def test_run_refusals(pix):
    """Odd half bases and strides, overlapping ranges, short strides, null pointers, n < 0 and wrong tensors are refused, and no refused call
    writes anything.  The source range covers all n frames, the destination range ceil(n / 2)."""
    import torch
    from pythoncrt_amd._lib import CrtfxError
    size, n = (3, 8), 4
    plan = _plan(size, pix, "tff", "linear")
    fb = 72 * (1 if pix == "u8" else 2)
    src = torch.zeros(n * fb + 16, dtype=torch.uint8, device=_dev())
    dst = torch.zeros(2 * fb + 16, dtype=torch.uint8, device=_dev())
    run, err = plan.lib.crtfx_interlace_run, plan.lib.crtfx_interlace_last_error
    st = torch.cuda.current_stream().cuda_stream
    sp, dp = src.data_ptr(), dst.data_ptr()
    if pix == "f16":
        assert run(plan._plan, sp + 1, fb, dp, fb, 1, st) == _lib.E_INVALID and b"even" in err(plan._plan)
        assert run(plan._plan, sp, fb, dp + 1, fb, 1, st) == _lib.E_INVALID and b"even" in err(plan._plan)
        assert run(plan._plan, sp, fb + 1, dp, fb, 2, st) == _lib.E_INVALID and b"even" in err(plan._plan)
        assert run(plan._plan, sp, fb, dp, fb + 1, 3, st) == _lib.E_INVALID and b"even" in err(plan._plan)
        assert run(plan._plan, sp, fb, dp, fb + 1, 2, st) == _lib.OK            # one frame written: the destination stride does not count
    assert run(plan._plan, sp, fb - 2, dp, fb, 2, st) == _lib.E_INVALID and b"strides" in err(plan._plan)
    assert run(plan._plan, sp, fb, dp, fb - 2, 3, st) == _lib.E_INVALID and b"strides" in err(plan._plan)
    assert run(plan._plan, sp, fb, dp, fb - 2, 2, st) == _lib.OK                # one frame written
    assert run(plan._plan, None, fb, dp, fb, 1, st) == _lib.E_INVALID and b"null" in err(plan._plan)
    assert run(plan._plan, sp, fb, None, fb, 1, st) == _lib.E_INVALID
    assert run(plan._plan, sp, fb, dp, fb, -1, st) == _lib.E_INVALID and b"n = -1" in err(plan._plan)
    # overlap: the destination inside the source's range, the source's last bytes on the destination's first, and the same buffer
    both = torch.zeros(n * 2 * fb + 8, dtype=torch.uint8, device=_dev())
    bp = both.data_ptr()
    for s_at, d_at in ((0, 0), (0, n * fb - 2), (2 * fb - 2, 0), (0, fb), (0, 3 * fb)):
        assert run(plan._plan, bp + s_at, fb, bp + d_at, fb, n, st) == _lib.E_INVALID and b"overlap" in err(plan._plan), (s_at, d_at)
    assert run(plan._plan, bp, fb, bp + n * fb, fb, n, st) == _lib.OK          # touching ranges do not overlap
    assert run(plan._plan, bp + 2 * fb, fb, bp, fb, n, st) == _lib.OK          # the destination's two frames end where the source begins
    torch.cuda.synchronize()
    assert int(dst.sum()) == 0 and int(src.sum()) == 0
    x = torch.zeros((n,) + size + (3,), dtype=_torch_dtype(pix), device=_dev())
    with pytest.raises(CrtfxError) as e:
        plan.run(x.to(torch.float32))
    assert e.value.code == _lib.E_UNSUPPORTED
    with pytest.raises(CrtfxError) as e:
        plan.run(x.to(torch.float16 if pix == "u8" else torch.uint8))
    assert e.value.code == _lib.E_UNSUPPORTED
    with pytest.raises(ValueError, match="frames must be"):
        plan.run(x[:, :2])
    with pytest.raises(ValueError, match="frames must be"):
        plan.run(x.cpu())
    for bad in (n, 1, 3):
        with pytest.raises(ValueError, match="out must be"):
            plan.run(x, out=torch.empty((bad,) + size + (3,), dtype=x.dtype, device=_dev()))
    with pytest.raises(CrtfxError) as e:
        plan.set_option(99, 1)
    assert e.value.code == _lib.E_INVALID and "option" in str(e.value)
    with pytest.raises(CrtfxError) as e:
        _plan((1, 8), pix, "tff", "none")
    assert e.value.code == _lib.E_INVALID and "h = 1" in str(e.value)
    plan.close()


@pytest.mark.parametrize("pix", list(DTYPES))
@pytest.mark.parametrize("order", model.ORDERS)
def test_deinterlacers_then_interlace_give_back_the_source(pix, order):
    """On the device: Deinterlace (both methods) and AdaptiveDeinterlace, both fields, then Interlace(none) of the same order: the source's
    bits, NaN payloads included; with the other order not."""
    import torch
    import pythoncrt_amd as pc
    size, n = (9, 24), 3
    src = _source(pix, (n,) + size + (3,), 21)
    x = torch.from_numpy(src).to(_dev())
    other = model.ORDERS[1 - model.ORDERS.index(order)]
    back, wrong = _plan(size, pix, order, "none"), _plan(size, pix, other, "none")
    plans = [pc.Deinterlace(_dev(), size, method=m, order=order, fields="both", dtype=_torch_dtype(pix)) for m in deint_model.METHODS]
    plans.append(pc.AdaptiveDeinterlace(_dev(), size, order=order, fields="both", dtype=_torch_dtype(pix)))
    for plan in plans:
        fields = plan.run(x)
        assert fields.shape[0] == 2 * n
        assert _same(back.run(fields).cpu().numpy(), src) == 0, type(plan).__name__
        assert _same(wrong.run(fields).cpu().numpy(), src) != 0
        plan.close()
    back.close()
    wrong.close()


@pytest.mark.parametrize("size,pix,order,lowpass", [
    ((480, 720), "u8", "bff", "linear"), ((480, 720), "f16", "tff", "complex"),
    ((1080, 1920), "u8", "tff", "complex"), ((1080, 1920), "f16", "bff", "linear")],
    ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v))
def test_a_full_size_batch(size, pix, order, lowpass):
    import torch
    n = 8
    src_np = model.noise(size[0], size[1], n=n, dtype=DTYPES[pix], seed=size[0])
    plan = _plan(size, pix, order, lowpass)
    out = plan.run(torch.from_numpy(src_np).to(_dev()))
    torch.cuda.synchronize()
    assert plan.plan() == {"interlace": _name(lowpass, pix, True), "frames": "8"}
    assert _same(out.cpu().numpy(), model.interlace(src_np, order, lowpass)) == 0
    plan.close()
