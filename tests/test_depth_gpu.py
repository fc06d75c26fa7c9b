"""The depth stage on the GPU (include/crtfx_depth.h) against tests/depth_model.py: both directions, both dithers, both paths.  Every
comparison is exact: no element may differ."""

import numpy as np
import pytest

from pythoncrt_amd import _lib
from tests import depth_model as model

pytestmark = pytest.mark.gpu

GUARD = 0xA5
SHAPES = [(1, 1), (1, 7), (3, 8), (2, 16), (9, 24), (17, 40), (5, 13), (8, 9)]         # 9 x 24: y & 7 wraps; 5 x 13 and 8 x 9: no multiple of 8
KINDS = [("widen", "none"), ("narrow", "none"), ("narrow", "ordered")]


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _plan(kind, size, dither="none", force=False):
    import pythoncrt_amd as pc
    return pc.Widen(_dev(), size, force_general=force) if kind == "widen" else pc.Narrow(_dev(), size, dither=dither, force_general=force)


def _halves(rng, shape):
    """Half frames that cross every rule: quarter codes, codes + 0.5, values past both ends, and a sprinkle of NaN, infinities and -0."""
    f = (rng.integers(-40, 1100, shape) / 4.0).astype(np.float16)
    flat = f.reshape(-1)
    pick = rng.integers(0, flat.size, max(1, flat.size // 16))
    flat[pick] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0, 255.5, 254.5, 0.5, 6e-8, 65504.0], dtype=np.float16), pick.size)
    return f


def _source(kind, rng, shape):
    return rng.integers(0, 256, shape, dtype=np.uint8) if kind == "widen" else _halves(rng, shape)


def _expected(kind, dither, src):
    return model.widen(src) if kind == "widen" else model.narrow(src, dither)


def _same(got, exp):
    """Bit for bit: halves are compared as their patterns."""
    assert got.dtype == exp.dtype and got.shape == exp.shape
    if got.dtype == np.float16:
        got, exp = got.view(np.uint16), exp.view(np.uint16)
    return int((got != exp).sum())


def _vec_expected(kind, w, src, dst, n, force=False):
    """The header's conditions, from the tensors' own addresses and strides."""
    if force or (kind == "narrow" and w % 8):
        return False
    if (src.data_ptr() | dst.data_ptr()) & 3:
        return False
    return n <= 1 or not ((src.stride(0) * src.element_size() | dst.stride(0) * dst.element_size()) & 3)


def _name(kind, dither, vec):
    path = "vec" if vec else "general"
    return f"k_widen<{path}>" if kind == "widen" else f"k_narrow<{dither},{path}>"


@pytest.mark.parametrize("force", [False, True], ids=["auto", "forced"])
@pytest.mark.parametrize("kind,dither", KINDS, ids=lambda v: str(v))
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_against_the_model(size, kind, dither, force):
    import torch
    rng = np.random.default_rng([size[0], size[1], len(kind), len(dither)])
    plan = _plan(kind, size, dither, force)
    for n in (1, 3):
        src = _source(kind, rng, (n,) + size + (3,))
        x = torch.from_numpy(src).to(_dev())
        out = plan.run(x)
        torch.cuda.synchronize()
        assert _same(out.cpu().numpy(), _expected(kind, dither, src)) == 0, (size, kind, dither, force, n)
        vec = _vec_expected(kind, size[1], x, out, n, force)
        assert plan.plan() == {"depth": _name(kind, dither, vec), "frames": str(n)}, plan.last_plan()
        if not force and n == 1:                                               # fresh allocations are aligned: the vec path wherever the width lets it
            assert vec == (kind == "widen" or size[1] % 8 == 0)
    plan.close()


@pytest.mark.parametrize("force", [False, True], ids=["vec", "general"])
@pytest.mark.parametrize("dither", model.DITHERS)
def test_narrow_every_half_pattern(dither, force):
    """All 65 536 half patterns over 64 x 1024 frames, four frames with the patterns rolled by different amounts, so that every pattern
    meets a dozen places of the threshold matrix."""
    import torch
    pats = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    frames = np.stack([np.concatenate([np.roll(pats, r + 8191 * k) for k in range(3)]) for r in (0, 1, 3077, 40000)]).view(np.float16).reshape(4, 64, 1024, 3)
    plan = _plan("narrow", (64, 1024), dither, force)
    out = plan.run(torch.from_numpy(frames).to(_dev()))
    torch.cuda.synchronize()
    assert plan.plan()["depth"] == _name("narrow", dither, not force)
    assert _same(out.cpu().numpy(), model.narrow(frames, dither)) == 0
    plan.close()


@pytest.mark.parametrize("dither", model.DITHERS)
def test_narrow_random_quarter_codes_and_widen_round_trip(dither):
    import torch
    rng = np.random.default_rng(77)
    q = (rng.integers(0, 1021, (2, 40, 72, 3)) / 4.0).astype(np.float16)
    plan = _plan("narrow", (40, 72), dither)
    out = plan.run(torch.from_numpy(q).to(_dev()))
    wide = _plan("widen", (40, 72)).run(out)
    back = plan.run(wide)
    torch.cuda.synchronize()
    assert _same(out.cpu().numpy(), model.narrow(q, dither)) == 0
    assert _same(wide.cpu().numpy(), model.widen(out.cpu().numpy())) == 0 and torch.equal(back, out)     # narrow(widen(u)) == u


def _guarded(n, frame_bytes, stride_bytes, offset, dtype):
    """(the guarded uint8 buffer, a [n, frame elements] view of `dtype` into it at byte `offset` with frame stride `stride_bytes`)."""
    import torch
    pad = 64
    total = pad + offset + (n - 1) * stride_bytes + frame_bytes + pad
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


@pytest.mark.parametrize("kind,dither", KINDS, ids=lambda v: str(v))
@pytest.mark.parametrize("size", [(3, 8), (9, 24), (5, 13)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_base_offset_inside_guards(size, kind, dither):
    """uint8 frames at byte offsets 0..3, half frames at 0 and 2, three frames with strides a few bytes longer than a frame: the bytes are
    the model's, the path is the one the header's conditions give, and no byte outside the frames changes."""
    import torch
    h, w = size
    rng = np.random.default_rng([h, w, 5])
    plan = _plan(kind, size, dither)
    u8_bytes, f16_bytes = h * w * 3, h * w * 6
    seen = set()
    for u8_off in range(4):
        for f16_off in (0, 2):
            for u8_gap, f16_gap in ((0, 0), (4, 8), (3, 2), (1, 2)):      # 5 x 13: 195 + 1 bytes is a stride the vec path takes
                n = 3
                src_np = _source(kind, rng, (n,) + size + (3,))
                if kind == "widen":
                    sb, s = _guarded(n, u8_bytes, u8_bytes + u8_gap, u8_off, torch.uint8)
                    db, d = _guarded(n, f16_bytes, f16_bytes + f16_gap, f16_off, torch.float16)
                else:
                    sb, s = _guarded(n, f16_bytes, f16_bytes + f16_gap, f16_off, torch.float16)
                    db, d = _guarded(n, u8_bytes, u8_bytes + u8_gap, u8_off, torch.uint8)
                s.copy_(torch.from_numpy(src_np.reshape(n, -1)).to(_dev()))
                s4 = s.as_strided((n, h, w, 3), (s.stride(0), w * 3, 3, 1))
                d4 = d.as_strided((n, h, w, 3), (d.stride(0), w * 3, 3, 1))
                plan.run(s4, out=d4)
                torch.cuda.synchronize()
                vec = _vec_expected(kind, w, s4, d4, n)
                seen.add(vec)
                assert plan.plan()["depth"] == _name(kind, dither, vec), (u8_off, f16_off, u8_gap, f16_gap, plan.last_plan())
                assert _same(d4.cpu().numpy(), _expected(kind, dither, src_np)) == 0, (u8_off, f16_off, u8_gap, f16_gap)
                assert _guards_intact(db, n, f16_bytes if kind == "widen" else u8_bytes, d.stride(0) * d.element_size(), f16_off if kind == "widen" else u8_off)
                assert _guards_intact(sb, n, u8_bytes if kind == "widen" else f16_bytes, s.stride(0) * s.element_size(), u8_off if kind == "widen" else f16_off)
    assert seen == ({False} if kind == "narrow" and w % 8 else {True, False})
    plan.close()


@pytest.mark.parametrize("kind,dither", KINDS, ids=lambda v: str(v))
def test_batches_with_unequal_strides_and_slices(kind, dither):
    """Slices of larger tensors: the source's batch stride and the destination's differ, and both exceed a frame."""
    import torch
    size, n = (9, 24), 4
    rng = np.random.default_rng(12)
    src_np = _source(kind, rng, (n, 2) + size + (3,))
    big_src = torch.from_numpy(src_np).to(_dev())
    dt = torch.float16 if kind == "widen" else torch.uint8
    big_dst = torch.zeros((n, 3) + size + (3,), dtype=dt, device=_dev())
    plan = _plan(kind, size, dither)
    out = plan.run(big_src[:, 1], out=big_dst[:, 2])
    torch.cuda.synchronize()
    assert out.data_ptr() == big_dst[:, 2].data_ptr() and plan.plan() == {"depth": _name(kind, dither, True), "frames": str(n)}
    assert _same(big_dst[:, 2].cpu().numpy(), _expected(kind, dither, src_np[:, 1])) == 0
    assert int(big_dst[:, :2].abs().sum()) == 0                                # the frames between: untouched
    with pytest.raises(ValueError, match="contiguous"):
        plan.run(torch.zeros((n,) + size + (6,), dtype=big_src.dtype, device=_dev())[..., ::2])      # the right shape, frames with holes
    plan.close()


@pytest.mark.parametrize("kind,dither", KINDS, ids=lambda v: str(v))
def test_no_frames_a_long_batch_and_the_call_forms(kind, dither):
    import torch
    size = (3, 8)
    rng = np.random.default_rng(65)
    plan = _plan(kind, size, dither)
    src_np = _source(kind, rng, (65,) + size + (3,))
    x = torch.from_numpy(src_np).to(_dev())
    out = plan.run(x)                                                          # 65 frames of 3 x 8 in one grid
    torch.cuda.synchronize()
    assert plan.plan() == {"depth": _name(kind, dither, True), "frames": "65"}
    assert _same(out.cpu().numpy(), _expected(kind, dither, src_np)) == 0
    assert torch.equal(plan(x).view(torch.uint8), plan.run(x).view(torch.uint8))       # plan(x) == plan.run(x)
    empty = plan.run(x[:0])
    assert tuple(empty.shape) == (0,) + size + (3,) and empty.dtype == out.dtype
    # n = 0 through the C entry point: nothing runs, nothing is written, nothing is asked of the pointers
    keep = out.clone()
    st = torch.cuda.current_stream().cuda_stream
    assert plan.lib.crtfx_depth_run(plan._plan, x.data_ptr(), 0, out.data_ptr(), 0, 0, st) == _lib.OK
    assert plan.lib.crtfx_depth_run(plan._plan, None, 0, None, 0, 0, st) == _lib.OK
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.uint8), keep.view(torch.uint8)) and plan.plan()["frames"] == "0"
    # force_general switches the plan string and not the bytes
    plan.force_general = True
    assert plan.force_general and plan.plan()["depth"] == _name(kind, dither, False)
    forced = plan.run(x)
    torch.cuda.synchronize()
    assert plan.plan() == {"depth": _name(kind, dither, False), "frames": "65"} and torch.equal(forced.view(torch.uint8), out.view(torch.uint8))
    plan.force_general = False
    assert plan.plan()["depth"] == _name(kind, dither, True)
    plan.close()


@pytest.mark.parametrize("kind,dither", KINDS[:2], ids=lambda v: str(v))
def test_run_refusals(kind, dither):
    """Odd half bases and strides, overlapping ranges, short strides, null pointers, n < 0 and wrong tensors are refused, and no refused call
    writes anything."""
    import torch
    from pythoncrt_amd._lib import CrtfxError
    size, n = (3, 8), 2
    plan = _plan(kind, size, dither)
    u8b, f16b = 72, 144
    sbytes, dbytes = (u8b, f16b) if kind == "widen" else (f16b, u8b)
    src = torch.zeros(n * sbytes + 16, dtype=torch.uint8, device=_dev())
    dst = torch.zeros(n * dbytes + 16, dtype=torch.uint8, device=_dev())
    run, err = plan.lib.crtfx_depth_run, plan.lib.crtfx_depth_last_error
    st = torch.cuda.current_stream().cuda_stream
    sp, dp = src.data_ptr(), dst.data_ptr()
    half_is_src = kind == "narrow"
    assert run(plan._plan, sp + half_is_src, sbytes, dp + (not half_is_src), dbytes, 1, st) == _lib.E_INVALID and b"even" in err(plan._plan)
    assert run(plan._plan, sp, sbytes + half_is_src, dp, dbytes + (not half_is_src), n, st) == _lib.E_INVALID and b"even" in err(plan._plan)     # an odd stride
    assert run(plan._plan, sp, sbytes - 2, dp, dbytes, n, st) == _lib.E_INVALID and b"strides" in err(plan._plan)
    assert run(plan._plan, sp, sbytes, dp, dbytes - 2, n, st) == _lib.E_INVALID and b"strides" in err(plan._plan)
    assert run(plan._plan, None, sbytes, dp, dbytes, 1, st) == _lib.E_INVALID and b"null" in err(plan._plan)
    assert run(plan._plan, sp, sbytes, None, dbytes, 1, st) == _lib.E_INVALID
    assert run(plan._plan, sp, sbytes, dp, dbytes, -1, st) == _lib.E_INVALID and b"n = -1" in err(plan._plan)
    # overlap: the destination inside the source's range, the source's last byte on the destination's first, and the same buffer
    both = torch.zeros(n * (sbytes + dbytes) + 8, dtype=torch.uint8, device=_dev())
    bp = both.data_ptr()
    for s_at, d_at in ((0, 0), (0, n * sbytes - 2), (n * dbytes - 2, 0), (0, sbytes)):
        assert run(plan._plan, bp + s_at, sbytes, bp + d_at, dbytes, n, st) == _lib.E_INVALID and b"overlap" in err(plan._plan), (s_at, d_at)
    assert run(plan._plan, bp, sbytes, bp + n * sbytes, dbytes, n, st) == _lib.OK      # touching ranges do not overlap
    torch.cuda.synchronize()
    assert int(dst.sum()) == 0 and int(src.sum()) == 0
    x = torch.zeros((n,) + size + (3,), dtype=torch.uint8 if kind == "widen" else torch.float16, device=_dev())
    with pytest.raises(CrtfxError) as e:
        plan.run(x.to(torch.float32))
    assert e.value.code == _lib.E_UNSUPPORTED
    with pytest.raises(ValueError, match="frames must be"):
        plan.run(x[:, :2])
    with pytest.raises(ValueError, match="out must be"):
        plan.run(x, out=torch.empty_like(x))
    with pytest.raises(CrtfxError) as e:
        plan.set_option(99, 1)
    assert e.value.code == _lib.E_INVALID and "option" in str(e.value)
    plan.close()


@pytest.mark.parametrize("kind,dither", KINDS, ids=lambda v: str(v))
def test_a_1080p_batch(kind, dither):
    import torch
    size, n = (1080, 1920), 4
    rng = np.random.default_rng(1080)
    src_np = rng.integers(0, 256, (n,) + size + (3,), dtype=np.uint8) if kind == "widen" else \
        (rng.integers(-8, 1040, (n,) + size + (3,), dtype=np.int16) / np.float32(4.0)).astype(np.float16)
    plan = _plan(kind, size, dither)
    out = plan.run(torch.from_numpy(src_np).to(_dev()))
    torch.cuda.synchronize()
    assert plan.plan() == {"depth": _name(kind, dither, True), "frames": "4"}
    assert _same(out.cpu().numpy(), _expected(kind, dither, src_np)) == 0
    plan.close()
