"""The deinterlace stage on the GPU (include/crtfx_deint.h) against tests/deint_model.py: both sample types, both methods, both orders, both
field modes, both paths.  Every comparison is exact: no element may differ."""
import itertools

import numpy as np
import pytest

from pythoncrt_amd import _lib
from tests import deint_model as model

pytestmark = pytest.mark.gpu

GUARD = 0xA5
# h = 2, 3: every missing row has one neighbour for some field; h even / odd: the last row is kept or made; w = 1, 6: no interior column;
# 7: exactly one; 8: one vec block; 16, 24, 40: the direction search crosses block boundaries; 23 x 40: the noise frame of test_deint_tables.py
SHAPES = [(2, 1), (3, 6), (2, 7), (3, 8), (4, 8), (5, 7), (6, 16), (7, 24), (2, 40), (23, 40)]
DTYPES = {"u8": np.uint8, "f16": np.float16}
COMBOS = list(itertools.product(model.METHODS, model.ORDERS, model.FIELDS))


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _torch_dtype(pix):
    import torch
    return torch.uint8 if pix == "u8" else torch.float16


def _plan(size, pix, method, order, fields, force=False):
    import pythoncrt_amd as pc
    return pc.Deinterlace(_dev(), size, method=method, order=order, fields=fields, dtype=_torch_dtype(pix), force_general=force)


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


def _vec_expected(w, src, dst, n, per, force=False):
    """The header's conditions, from the tensors' own addresses and strides."""
    if force or w % 8 or (src.data_ptr() | dst.data_ptr()) & 3:
        return False
    if n > 1 and (src.stride(0) * src.element_size()) & 3:
        return False
    return n * per <= 1 or not (dst.stride(0) * dst.element_size()) & 3


def _name(method, pix, fields, vec):
    return f"k_deint<{method},{pix},{fields},{'vec' if vec else 'general'}>"


@pytest.mark.parametrize("force", [False, True], ids=["auto", "forced"])
@pytest.mark.parametrize("pix", list(DTYPES))
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_against_the_model(size, pix, force):
    import torch
    for n in (1, 3):
        src = model.noise(size[0], size[1], n=n, dtype=DTYPES[pix]) if size == (23, 40) else _source(pix, (n,) + size + (3,), [size[0], size[1], n])
        x = torch.from_numpy(src).to(_dev())
        for method, order, fields in COMBOS:
            plan = _plan(size, pix, method, order, fields, force)
            out = plan.run(x)
            torch.cuda.synchronize()
            per = 2 if fields == "both" else 1
            assert plan.frames_out == per and tuple(out.shape) == (n * per,) + size + (3,)
            assert _same(out.cpu().numpy(), model.deinterlace(src, method, order, fields)) == 0, (size, pix, method, order, fields, force, n)
            vec = _vec_expected(size[1], x, out, n, per, force)
            assert plan.plan() == {"deint": _name(method, pix, fields, vec), "frames": str(n)}, plan.last_plan()
            if not force:                                                      # fresh allocations are aligned: the vec path wherever the width lets it
                assert vec == (size[1] % 8 == 0)
            plan.close()


@pytest.mark.parametrize("force", [False, True], ids=["vec", "general"])
@pytest.mark.parametrize("method", model.METHODS)
def test_every_half_pattern_kept_and_interpolated(method, force):
    """All 65 536 half patterns in each of the three rows of a 3 x 21848 frame, rolled differently: under BOTH every pattern is kept once
    (its bits survive), feeds the interpolation of row 1 from rows 0 and 2, and is the one neighbour rows 0 and 2 are copied from."""
    import torch
    w = 21848                                                                   # 8 * 2731 pixels: 65 544 samples per row
    pats = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    rows = [np.concatenate([np.roll(pats, r), pats[:8]]) for r in (0, 40001, 12345)]
    src = np.stack(rows).view(np.float16).reshape(1, 3, w, 3)
    for order in model.ORDERS:
        plan = _plan((3, w), "f16", method, order, "both", force)
        out = plan.run(torch.from_numpy(src).to(_dev()))
        torch.cuda.synchronize()
        assert plan.plan()["deint"] == _name(method, "f16", "both", not force)
        got = out.cpu().numpy()
        assert _same(got, model.deinterlace(src, method, order, "both")) == 0
        first = model.ORDERS.index(order)
        assert np.array_equal(model.bits(got[0, first::2]), model.bits(src[0, first::2]))
        assert np.array_equal(model.bits(got[1, 1 - first::2]), model.bits(src[0, 1 - first::2]))
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


@pytest.mark.parametrize("method", model.METHODS)
@pytest.mark.parametrize("pix", list(DTYPES))
@pytest.mark.parametrize("size", [(3, 8), (9, 24), (5, 13)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_base_offset_inside_guards(size, pix, method):
    """uint8 frames at byte offsets 0..3, half frames at 0 and 2, three source frames, source and destination strides that differ and are a
    few bytes longer than a frame: the bytes are the model's, the path is the one the header's conditions give, and no byte outside the
    frames changes, in the source or in the destination."""
    import torch
    h, w = size
    dt, item = _torch_dtype(pix), (1 if pix == "u8" else 2)
    fb = h * w * 3 * item
    offsets = range(4) if pix == "u8" else (0, 2)
    seen = set()
    n = 3
    for fields in model.FIELDS:
        per = 2 if fields == "both" else 1
        plan = _plan(size, pix, method, "bff", fields)
        for s_off, d_off in itertools.product(offsets, offsets):
            for s_gap, d_gap in ((0, 4), (8, 0), (2, 6), (4, 8)) if pix == "f16" else ((0, 4), (8, 0), (3, 1), (1, 4)):
                src_np = _source(pix, (n,) + size + (3,), [h, w, s_off, d_off, s_gap])
                sb, s = _guarded(n, fb, fb + s_gap, s_off, dt)
                db, d = _guarded(n * per, fb, fb + d_gap, d_off, dt)
                s.copy_(torch.from_numpy(src_np.reshape(n, -1)).to(_dev()))
                s4 = s.as_strided((n, h, w, 3), (s.stride(0), w * 3, 3, 1))
                d4 = d.as_strided((n * per, h, w, 3), (d.stride(0), w * 3, 3, 1))
                plan.run(s4, out=d4)
                torch.cuda.synchronize()
                vec = _vec_expected(w, s4, d4, n, per)
                seen.add(vec)
                assert plan.plan()["deint"] == _name(method, pix, fields, vec), (s_off, d_off, s_gap, d_gap, plan.last_plan())
                assert _same(d4.cpu().numpy(), model.deinterlace(src_np, method, "bff", fields)) == 0, (fields, s_off, d_off, s_gap, d_gap)
                assert _guards_intact(db, n * per, fb, fb + d_gap, d_off) and _guards_intact(sb, n, fb, fb + s_gap, s_off)
                assert _same(s4.cpu().numpy(), src_np) == 0
        plan.close()
    assert seen == ({False} if w % 8 else {True, False})


@pytest.mark.parametrize("pix", list(DTYPES))
def test_one_source_frame_under_both_asks_for_an_aligned_destination_stride(pix):
    """n = 1 under BOTH writes two frames: the destination stride counts, the source stride does not."""
    import torch
    size, item = (4, 8), (1 if pix == "u8" else 2)
    fb = 4 * 8 * 3 * item
    src_np = _source(pix, (1,) + size + (3,), 11)
    plan = _plan(size, pix, "edge", "tff", "both")
    for d_gap, vec in ((0, True), (4, True), (2, False), (6, False)):
        sb, s = _guarded(1, fb, fb + 2, 0, _torch_dtype(pix))
        db, d = _guarded(2, fb, fb + d_gap, 0, _torch_dtype(pix))
        s.copy_(torch.from_numpy(src_np.reshape(1, -1)).to(_dev()))
        d4 = d.as_strided((2,) + size + (3,), (d.stride(0), 24, 3, 1))
        plan.run(s.as_strided((1,) + size + (3,), (s.stride(0), 24, 3, 1)), out=d4)
        torch.cuda.synchronize()
        assert plan.plan() == {"deint": _name("edge", pix, "both", vec), "frames": "1"}
        assert _same(d4.cpu().numpy(), model.deinterlace(src_np, "edge", "tff", "both")) == 0 and _guards_intact(db, 2, fb, fb + d_gap, 0)
    plan.close()


@pytest.mark.parametrize("fields", model.FIELDS)
@pytest.mark.parametrize("pix", list(DTYPES))
def test_batches_with_unequal_strides_and_slices(pix, fields):
    """Slices of larger tensors: the source's batch stride and the destination's differ, and both exceed a frame."""
    import torch
    size, n = (9, 24), 4
    per = 2 if fields == "both" else 1
    src_np = _source(pix, (n, 2) + size + (3,), 12)
    big_src = torch.from_numpy(src_np).to(_dev())
    big_dst = torch.zeros((n * per, 3) + size + (3,), dtype=_torch_dtype(pix), device=_dev())
    plan = _plan(size, pix, "edge", "tff", fields)
    out = plan.run(big_src[:, 1], out=big_dst[:, 2])
    torch.cuda.synchronize()
    assert out.data_ptr() == big_dst[:, 2].data_ptr() and plan.plan() == {"deint": _name("edge", pix, fields, True), "frames": str(n)}
    assert _same(big_dst[:, 2].cpu().numpy(), model.deinterlace(src_np[:, 1], "edge", "tff", fields)) == 0
    assert int(big_dst[:, :2].view(torch.uint8).sum()) == 0                     # the frames between: untouched
    with pytest.raises(ValueError, match="contiguous"):
        plan.run(torch.zeros((n,) + size + (6,), dtype=big_src.dtype, device=_dev())[..., ::2])      # the right shape, frames with holes
    plan.close()


@pytest.mark.parametrize("method,fields", list(itertools.product(model.METHODS, model.FIELDS)))
@pytest.mark.parametrize("pix", list(DTYPES))
def test_no_frames_a_long_batch_and_the_call_forms(pix, method, fields):
    import torch
    size = (3, 8)
    per = 2 if fields == "both" else 1
    plan = _plan(size, pix, method, "tff", fields)
    src_np = _source(pix, (65,) + size + (3,), 65)
    x = torch.from_numpy(src_np).to(_dev())
    out = plan.run(x)                                                          # 65 source frames of 3 x 8 in one grid
    torch.cuda.synchronize()
    assert plan.plan() == {"deint": _name(method, pix, fields, True), "frames": "65"}
    assert _same(out.cpu().numpy(), model.deinterlace(src_np, method, "tff", fields)) == 0
    assert torch.equal(plan(x).view(torch.uint8), plan.run(x).view(torch.uint8))       # plan(x) == plan.run(x)
    empty = plan.run(x[:0])
    assert tuple(empty.shape) == (0,) + size + (3,) and empty.dtype == out.dtype
    keep = out.clone()
    assert plan.run(x[:0], out=out[:0]).data_ptr() == out[:0].data_ptr()       # n = 0: `out` comes back untouched
    # n = 0 through the C entry point: nothing runs, nothing is written, nothing is asked of the pointers
    st = torch.cuda.current_stream().cuda_stream
    assert plan.lib.crtfx_deint_run(plan._plan, x.data_ptr(), 0, out.data_ptr(), 0, 0, st) == _lib.OK
    assert plan.lib.crtfx_deint_run(plan._plan, None, 0, None, 0, 0, st) == _lib.OK
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.uint8), keep.view(torch.uint8)) and plan.plan()["frames"] == "0"
    # force_general switches the plan string and not the bytes
    plan.force_general = True
    assert plan.force_general and plan.plan()["deint"] == _name(method, pix, fields, False)
    forced = plan.run(x)
    torch.cuda.synchronize()
    assert plan.plan() == {"deint": _name(method, pix, fields, False), "frames": "65"} and torch.equal(forced.view(torch.uint8), out.view(torch.uint8))
    plan.force_general = False
    assert plan.plan()["deint"] == _name(method, pix, fields, True)
    plan.close()


@pytest.mark.parametrize("fields", model.FIELDS)
@pytest.mark.parametrize("pix", list(DTYPES))
def test_run_refusals(pix, fields):
    """Odd half bases and strides, overlapping ranges, short strides, null pointers, n < 0 and wrong tensors are refused, and no refused call
    writes anything."""
    import torch
    from pythoncrt_amd._lib import CrtfxError
    size, n = (3, 8), 2
    per = 2 if fields == "both" else 1
    plan = _plan(size, pix, "linear", "tff", fields)
    fb = 72 * (1 if pix == "u8" else 2)
    src = torch.zeros(n * fb + 16, dtype=torch.uint8, device=_dev())
    dst = torch.zeros(n * per * fb + 16, dtype=torch.uint8, device=_dev())
    run, err = plan.lib.crtfx_deint_run, plan.lib.crtfx_deint_last_error
    st = torch.cuda.current_stream().cuda_stream
    sp, dp = src.data_ptr(), dst.data_ptr()
    if pix == "f16":
        assert run(plan._plan, sp + 1, fb, dp, fb, 1, st) == _lib.E_INVALID and b"even" in err(plan._plan)
        assert run(plan._plan, sp, fb, dp + 1, fb, 1, st) == _lib.E_INVALID and b"even" in err(plan._plan)
        assert run(plan._plan, sp, fb + 1, dp, fb, n, st) == _lib.E_INVALID and b"even" in err(plan._plan)
        assert run(plan._plan, sp, fb, dp, fb + 1, n, st) == _lib.E_INVALID and b"even" in err(plan._plan)
    assert run(plan._plan, sp, fb - 2, dp, fb, n, st) == _lib.E_INVALID and b"strides" in err(plan._plan)
    assert run(plan._plan, sp, fb, dp, fb - 2, n, st) == _lib.E_INVALID and b"strides" in err(plan._plan)
    if fields == "both":                                                       # one source frame, two frames written: the destination stride counts
        assert run(plan._plan, sp, 0, dp, fb - 2, 1, st) == _lib.E_INVALID and b"strides" in err(plan._plan)
    assert run(plan._plan, None, fb, dp, fb, 1, st) == _lib.E_INVALID and b"null" in err(plan._plan)
    assert run(plan._plan, sp, fb, None, fb, 1, st) == _lib.E_INVALID
    assert run(plan._plan, sp, fb, dp, fb, -1, st) == _lib.E_INVALID and b"n = -1" in err(plan._plan)
    # overlap: the destination inside the source's range, the source's last bytes on the destination's first, and the same buffer
    both = torch.zeros(n * (1 + per) * fb + 8, dtype=torch.uint8, device=_dev())
    bp = both.data_ptr()
    for s_at, d_at in ((0, 0), (0, n * fb - 2), (n * per * fb - 2, 0), (0, fb)):
        assert run(plan._plan, bp + s_at, fb, bp + d_at, fb, n, st) == _lib.E_INVALID and b"overlap" in err(plan._plan), (s_at, d_at)
    assert run(plan._plan, bp, fb, bp + n * fb, fb, n, st) == _lib.OK          # touching ranges do not overlap
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
    with pytest.raises(ValueError, match="out must be"):
        plan.run(x, out=torch.empty((n * per + 1,) + size + (3,), dtype=x.dtype, device=_dev()))
    with pytest.raises(CrtfxError) as e:
        plan.set_option(99, 1)
    assert e.value.code == _lib.E_INVALID and "option" in str(e.value)
    with pytest.raises(CrtfxError) as e:
        _plan((1, 8), pix, "linear", "tff", fields)
    assert e.value.code == _lib.E_INVALID and "h = 1" in str(e.value)
    plan.close()


@pytest.mark.parametrize("size,pix,method,order,fields", [
    ((480, 720), "u8", "edge", "bff", "both"), ((480, 720), "f16", "edge", "tff", "both"), ((480, 720), "f16", "linear", "bff", "first"),
    ((1080, 1920), "u8", "edge", "tff", "both"), ((1080, 1920), "f16", "edge", "bff", "first"), ((1080, 1920), "u8", "linear", "bff", "both")],
    ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v))
def test_a_full_size_batch(size, pix, method, order, fields):
    import torch
    n = 4
    src_np = model.noise(size[0], size[1], n=n, dtype=DTYPES[pix], seed=size[0])
    plan = _plan(size, pix, method, order, fields)
    out = plan.run(torch.from_numpy(src_np).to(_dev()))
    torch.cuda.synchronize()
    assert plan.plan() == {"deint": _name(method, pix, fields, True), "frames": "4"}
    assert _same(out.cpu().numpy(), model.deinterlace(src_np, method, order, fields)) == 0
    plan.close()
