"""The motion-adaptive deinterlace stage on the GPU (include/crtfx_adeint.h) against tests/adeint_model.py: both sample types, both orders,
both field modes, both paths, with and without a previous frame.  Every comparison is exact: no element may differ."""
import itertools

import numpy as np
import pytest

from pythoncrt_amd import _lib
from tests import adeint_model as model
from tests import deint_model as dm

pytestmark = pytest.mark.gpu

GUARD = 0xA5
# the shapes of test_deint_gpu.py: h = 2, 3: every made row has one neighbour for some field; w = 1, 6: no interior column; 7: exactly one;
# 8: one vec block; 16, 24, 40: the direction search crosses block boundaries
SHAPES = [(2, 1), (3, 6), (2, 7), (3, 8), (4, 8), (5, 7), (6, 16), (7, 24), (2, 40), (23, 40)]
DTYPES = {"u8": np.uint8, "f16": np.float16}
COMBOS = list(itertools.product(model.ORDERS, model.FIELDS))
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 255.5, 254.875, 0.125, 6e-8, 65504.0, 100.1, -3.0], dtype=np.float16)


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _torch_dtype(pix):
    import torch
    return torch.uint8 if pix == "u8" else torch.float16


def _plan(size, pix, order, fields, force=False):
    import pythoncrt_amd as pc
    return pc.AdaptiveDeinterlace(_dev(), size, order=order, fields=fields, dtype=_torch_dtype(pix), force_general=force)


def scene(pix, n, h, w, seed):
    """(frames [n, h, w, 3], prev [h, w, 3]): still and changed regions mixed (adeint_model.scene); half frames also carry patterns that
    cross every rule of the quantiser — values between quarter codes and past both ends, NaN, infinities, -0 — in C and in P alike."""
    frames, prev = model.scene(n, h, w, DTYPES[pix], seed=seed, still=0.6)
    if pix == "f16":
        rng = np.random.default_rng(seed + 1)
        seq = np.concatenate([prev[None], frames])
        flat = seq.reshape(-1)
        pick = rng.integers(0, flat.size, max(1, flat.size // 16))
        flat[pick] = rng.choice(SPECIALS, pick.size)
        frames, prev = seq[1:], seq[0]
    return np.ascontiguousarray(frames), np.ascontiguousarray(prev)


clamp_classes = model.clamp_classes


def _same(got, exp):
    """Bit for bit: halves are compared as their patterns."""
    assert got.dtype == exp.dtype and got.shape == exp.shape, (got.dtype, exp.dtype, got.shape, exp.shape)
    return int((dm.bits(got) != dm.bits(exp)).sum())


def _vec_expected(w, src, dst, n, per, prev=None, force=False):
    """The header's conditions, from the tensors' own addresses and strides."""
    if force or w % 8 or (src.data_ptr() | dst.data_ptr() | (0 if prev is None else prev.data_ptr())) & 3:
        return False
    if n > 1 and (src.stride(0) * src.element_size()) & 3:
        return False
    return n * per <= 1 or not (dst.stride(0) * dst.element_size()) & 3


def _name(pix, fields, vec):
    return f"k_adeint<{pix},{fields},{'vec' if vec else 'general'}>"


@pytest.mark.parametrize("force", [False, True], ids=["auto", "forced"])
@pytest.mark.parametrize("pix", list(DTYPES))
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_against_the_model(size, pix, force):
    import torch
    seen = set()
    for n in (1, 3, 5):
        src, prev = scene(pix, n, size[0], size[1], seed=size[0] * 1000 + size[1] * 10 + n)
        x, pv = torch.from_numpy(src).to(_dev()), torch.from_numpy(prev).to(_dev())
        for order, fields in COMBOS:
            plan = _plan(size, pix, order, fields, force)
            per = 2 if fields == "both" else 1
            for p_np, p_t in ((None, None), (prev, pv)):
                out = plan.run(x, prev=p_t)
                torch.cuda.synchronize()
                exp, parts = model.adaptive_parts(src, p_np, order, fields)
                seen |= clamp_classes(parts)
                assert plan.frames_out == per and tuple(out.shape) == (n * per,) + size + (3,)
                assert _same(out.cpu().numpy(), exp) == 0, (size, pix, order, fields, force, n, p_np is None)
                vec = _vec_expected(size[1], x, out, n, per, p_t, force)
                assert plan.plan() == {"adeint": _name(pix, fields, vec), "frames": str(n)}, plan.last_plan()
                if not force:                                                  # fresh allocations are aligned: the vec path wherever the width lets it
                    assert vec == (size[1] % 8 == 0)
            plan.close()
    assert seen == {"weave", "held", "edge"}, seen                             # both sides of the clamp and m = 0, in every case


@pytest.mark.parametrize("force", [False, True], ids=["vec", "general"])
def test_every_half_pattern_in_c_and_in_p(force):
    """All 65 536 half patterns in each of the three rows of a 3 x 21848 frame C and of its previous frame P, each row rolled differently:
    under BOTH every pattern is kept once (its bits survive), is the centre of a clamp, feeds EDGE's rows and m from either frame."""
    import torch
    w = 21848                                                                   # 8 * 2731 pixels: 65 544 samples per row
    pats = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    rows = lambda rolls: np.stack([np.concatenate([np.roll(pats, r), pats[:8]]) for r in rolls]).view(np.float16).reshape(3, w, 3)   # noqa: E731
    src, prev = rows((0, 40001, 12345))[None], rows((7, 40001, 333))            # row 1: the same patterns in both, m from the neighbours alone
    x, pv = torch.from_numpy(src).to(_dev()), torch.from_numpy(prev).to(_dev())
    for order in model.ORDERS:
        plan = _plan((3, w), "f16", order, "both", force)
        out = plan.run(x, prev=pv)
        torch.cuda.synchronize()
        assert plan.plan()["adeint"] == _name("f16", "both", not force)
        got = out.cpu().numpy()
        assert _same(got, model.adaptive(src, prev, order, "both")) == 0
        first = model.ORDERS.index(order)
        assert np.array_equal(dm.bits(got[0, first::2]), dm.bits(src[0, first::2]))
        assert np.array_equal(dm.bits(got[1, 1 - first::2]), dm.bits(src[0, 1 - first::2]))
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


@pytest.mark.parametrize("pix", list(DTYPES))
@pytest.mark.parametrize("size", [(3, 8), (9, 24)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_prev_at_every_offset_and_inside_the_source(size, pix):
    """prev at byte offsets 0..3 (0, 2 for halves) inside a guarded buffer: the general path whenever it is not a multiple of 4, the same
    bytes either way.  Then prev a view of the source batch: its last frame, and the frame in front of a slice."""
    import torch
    h, w = size
    dt, item = _torch_dtype(pix), (1 if pix == "u8" else 2)
    fb = h * w * 3 * item
    src, prev = scene(pix, 3, h, w, seed=h + w)
    x = torch.from_numpy(src).to(_dev())
    for order, fields in COMBOS:
        plan = _plan(size, pix, order, fields)
        exp = model.adaptive(src, prev, order, fields)
        for off in (range(4) if pix == "u8" else (0, 2)):
            pbuf, pview = _guarded(1, fb, fb, off, dt)
            pview.copy_(torch.from_numpy(prev.reshape(1, -1)).to(_dev()))
            p_t = pview[0].view(h, w, 3)
            assert p_t.data_ptr() % 4 == off
            out = plan.run(x, prev=p_t)
            torch.cuda.synchronize()
            assert plan.plan()["adeint"] == _name(pix, fields, off == 0), (off, plan.last_plan())
            assert _same(out.cpu().numpy(), exp) == 0, (order, fields, off)
            assert _guards_intact(pbuf, 1, fb, fb, off) and _same(p_t.cpu().numpy(), prev) == 0
        out = plan.run(x, prev=x[2])                                           # inside the source range
        torch.cuda.synchronize()
        assert _same(out.cpu().numpy(), model.adaptive(src, src[2], order, fields)) == 0
        out = plan.run(x[1:], prev=x[0])                                       # the stateless call continuing a batch: frames 1.. of the whole
        torch.cuda.synchronize()
        per = 2 if fields == "both" else 1
        assert _same(out.cpu().numpy(), exp[per:]) == 0
        plan.close()


@pytest.mark.parametrize("pix", list(DTYPES))
@pytest.mark.parametrize("size", [(3, 8), (9, 24), (5, 13)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_base_offset_inside_guards(size, pix):
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
    src_np, prev = scene(pix, n, h, w, seed=7 * h + w)
    pv = torch.from_numpy(prev).to(_dev())
    for fields in model.FIELDS:
        per = 2 if fields == "both" else 1
        plan = _plan(size, pix, "bff", fields)
        exp = model.adaptive(src_np, prev, "bff", fields)
        for s_off, d_off in itertools.product(offsets, offsets):
            for s_gap, d_gap in ((0, 4), (8, 0), (2, 6), (4, 8)) if pix == "f16" else ((0, 4), (8, 0), (3, 1), (1, 4)):
                sb, s = _guarded(n, fb, fb + s_gap, s_off, dt)
                db, d = _guarded(n * per, fb, fb + d_gap, d_off, dt)
                s.copy_(torch.from_numpy(src_np.reshape(n, -1)).to(_dev()))
                s4 = s.as_strided((n, h, w, 3), (s.stride(0), w * 3, 3, 1))
                d4 = d.as_strided((n * per, h, w, 3), (d.stride(0), w * 3, 3, 1))
                plan.run(s4, out=d4, prev=pv)
                torch.cuda.synchronize()
                vec = _vec_expected(w, s4, d4, n, per, pv)
                seen.add(vec)
                assert plan.plan()["adeint"] == _name(pix, fields, vec), (s_off, d_off, s_gap, d_gap, plan.last_plan())
                assert _same(d4.cpu().numpy(), exp) == 0, (fields, s_off, d_off, s_gap, d_gap)
                assert _guards_intact(db, n * per, fb, fb + d_gap, d_off) and _guards_intact(sb, n, fb, fb + s_gap, s_off)
                assert _same(s4.cpu().numpy(), src_np) == 0
        plan.close()
    assert seen == ({False} if w % 8 else {True, False})


@pytest.mark.parametrize("fields", model.FIELDS)
@pytest.mark.parametrize("pix", list(DTYPES))
def test_no_frames_a_long_batch_and_the_call_forms(pix, fields):
    import torch
    size = (3, 8)
    plan = _plan(size, pix, "tff", fields)
    src_np, prev = scene(pix, 65, 3, 8, seed=65)
    x, pv = torch.from_numpy(src_np).to(_dev()), torch.from_numpy(prev).to(_dev())
    out = plan.run(x, prev=pv)                                                 # 65 source frames of 3 x 8 in one grid
    torch.cuda.synchronize()
    assert plan.plan() == {"adeint": _name(pix, fields, True), "frames": "65"}
    assert _same(out.cpu().numpy(), model.adaptive(src_np, prev, "tff", fields)) == 0
    assert torch.equal(plan(x).view(torch.uint8), plan.run(x).view(torch.uint8))       # plan(x) == plan.run(x): no previous frame
    empty = plan.run(x[:0], prev=pv)
    assert tuple(empty.shape) == (0,) + size + (3,) and empty.dtype == out.dtype
    keep = out.clone()
    assert plan.run(x[:0], out=out[:0]).data_ptr() == out[:0].data_ptr()       # n = 0: `out` comes back untouched
    st = torch.cuda.current_stream().cuda_stream
    run = plan.lib.crtfx_adeint_run
    assert run(plan._plan, pv.data_ptr(), x.data_ptr(), 0, out.data_ptr(), 0, 0, st) == _lib.OK
    assert run(plan._plan, None, None, 0, None, 0, 0, st) == _lib.OK
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.uint8), keep.view(torch.uint8)) and plan.plan()["frames"] == "0"
    plan.force_general = True                                                  # switches the plan string and not the bytes
    assert plan.force_general and plan.plan()["adeint"] == _name(pix, fields, False)
    forced = plan.run(x, prev=pv)
    torch.cuda.synchronize()
    assert plan.plan() == {"adeint": _name(pix, fields, False), "frames": "65"} and torch.equal(forced.view(torch.uint8), out.view(torch.uint8))
    plan.force_general = False
    assert plan.plan()["adeint"] == _name(pix, fields, True)
    plan.close()


@pytest.mark.parametrize("force", [False, True], ids=["vec", "general"])
def test_a_batch_past_one_launch_group(force):
    """32 769 frames of 2 x 8 uint8: the last frame is a launch of its own and takes frame 32 767 as its previous frame.  The frames on either
    side of the boundary and a seeded handful of others, each against the model of its own frame pair."""
    import torch
    n, size = 32769, (2, 8)
    rng = np.random.default_rng(32769)
    base = rng.integers(0, 256, (1,) + size + (3,), dtype=np.uint8)
    src = np.repeat(base, n, axis=0)
    change = rng.random((n,) + size) < 0.3                                     # every frame: the one before it with some pixels redrawn
    fresh = rng.integers(0, 256, (n,) + size + (3,), dtype=np.uint8)
    for i in range(1, n):
        src[i] = np.where(change[i][..., None], fresh[i], src[i - 1])
    x = torch.from_numpy(src).to(_dev())
    plan = _plan(size, "u8", "tff", "both", force)
    out = plan.run(x)
    torch.cuda.synchronize()
    assert plan.plan() == {"adeint": _name("u8", "both", not force), "frames": str(n)}
    got = out.cpu().numpy()
    picks = sorted({0, 1, 32766, 32767, 32768} | set(int(v) for v in rng.integers(2, 32766, 12)))
    for i in picks:
        exp = model.adaptive(src[i:i + 1], src[i - 1] if i else None, "tff", "both")
        assert _same(got[2 * i:2 * i + 2], exp) == 0, i
    assert not np.array_equal(got[2 * 32768:], dm.deinterlace(src[32768:], "edge", "tff", "both"))    # the boundary frame HAS a previous frame
    plan.close()


@pytest.mark.parametrize("fields", model.FIELDS)
@pytest.mark.parametrize("pix", list(DTYPES))
def test_run_refusals(pix, fields):
    """Every refusal of crtfx_deint_run, an odd prev_frame for half frames and a prev_frame that overlaps the destination; no refused call
    writes anything."""
    import torch
    from pythoncrt_amd._lib import CrtfxError
    size, n = (3, 8), 2
    per = 2 if fields == "both" else 1
    plan = _plan(size, pix, "tff", fields)
    fb = 72 * (1 if pix == "u8" else 2)
    src = torch.zeros(n * fb + 16, dtype=torch.uint8, device=_dev())
    dst = torch.zeros(n * per * fb + 16, dtype=torch.uint8, device=_dev())
    prv = torch.zeros(fb + 16, dtype=torch.uint8, device=_dev())
    run, err = plan.lib.crtfx_adeint_run, plan.lib.crtfx_adeint_last_error
    st = torch.cuda.current_stream().cuda_stream
    sp, dp, pp = src.data_ptr(), dst.data_ptr(), prv.data_ptr()
    if pix == "f16":
        assert run(plan._plan, pp, sp + 1, fb, dp, fb, 1, st) == _lib.E_INVALID and b"even" in err(plan._plan)
        assert run(plan._plan, pp, sp, fb, dp + 1, fb, 1, st) == _lib.E_INVALID and b"even" in err(plan._plan)
        assert run(plan._plan, pp, sp, fb + 1, dp, fb, n, st) == _lib.E_INVALID and b"even" in err(plan._plan)
        assert run(plan._plan, pp, sp, fb, dp, fb + 1, n, st) == _lib.E_INVALID and b"even" in err(plan._plan)
        assert run(plan._plan, pp + 1, sp, fb, dp, fb, n, st) == _lib.E_INVALID and b"even prev_frame" in err(plan._plan)
    assert run(plan._plan, pp, sp, fb - 2, dp, fb, n, st) == _lib.E_INVALID and b"strides" in err(plan._plan)
    assert run(plan._plan, pp, sp, fb, dp, fb - 2, n, st) == _lib.E_INVALID and b"strides" in err(plan._plan)
    if fields == "both":
        assert run(plan._plan, pp, sp, 0, dp, fb - 2, 1, st) == _lib.E_INVALID and b"strides" in err(plan._plan)
    assert run(plan._plan, pp, None, fb, dp, fb, 1, st) == _lib.E_INVALID and b"null" in err(plan._plan)
    assert run(plan._plan, pp, sp, fb, None, fb, 1, st) == _lib.E_INVALID
    assert run(plan._plan, pp, sp, fb, dp, fb, -1, st) == _lib.E_INVALID and b"n = -1" in err(plan._plan)
    both = torch.zeros(n * (1 + per) * fb + 8, dtype=torch.uint8, device=_dev())
    bp = both.data_ptr()
    for s_at, d_at in ((0, 0), (0, n * fb - 2), (n * per * fb - 2, 0), (0, fb)):
        assert run(plan._plan, pp, bp + s_at, fb, bp + d_at, fb, n, st) == _lib.E_INVALID and b"source and destination overlap" in err(plan._plan), (s_at, d_at)
    # prev_frame against the destination [dp, dp + n * per * fb): its first bytes, its last, inside, the same base
    for p_at in (dp, dp + n * per * fb - 2, dp + fb, dp - fb + 2):
        assert run(plan._plan, p_at, sp, fb, dp, fb, n, st) == _lib.E_INVALID and b"prev_frame and destination overlap" in err(plan._plan), p_at - dp
    assert run(plan._plan, bp + n * (1 + per) * fb - fb, bp, fb, bp + n * fb, fb, n, st) == _lib.E_INVALID       # prev inside the destination's tail
    assert run(plan._plan, bp, bp, fb, bp + n * fb, fb, n, st) == _lib.OK      # touching ranges do not overlap; prev inside the source range
    assert run(plan._plan, bp + fb, bp, fb, bp + n * fb, fb, n, st) == _lib.OK
    torch.cuda.synchronize()
    assert int(dst.sum()) == 0 and int(src.sum()) == 0 and int(prv.sum()) == 0
    x = torch.zeros((n,) + size + (3,), dtype=_torch_dtype(pix), device=_dev())
    with pytest.raises(CrtfxError) as e:
        plan.run(x.to(torch.float32))
    assert e.value.code == _lib.E_UNSUPPORTED
    with pytest.raises(ValueError, match="frames must be"):
        plan.run(x[:, :2])
    with pytest.raises(ValueError, match="frames must be"):
        plan.run(x.cpu())
    with pytest.raises(ValueError, match="out must be"):
        plan.run(x, out=torch.empty((n * per + 1,) + size + (3,), dtype=x.dtype, device=_dev()))
    for bad in (x, x[0, :2], x[0].cpu(), x[0].to(torch.float32), torch.zeros(size + (6,), dtype=x.dtype, device=_dev())[..., ::2]):
        with pytest.raises(ValueError, match="prev must be"):
            plan.run(x, prev=bad)
    with pytest.raises(ValueError, match="contiguous"):
        plan.run(torch.zeros((n,) + size + (6,), dtype=x.dtype, device=_dev())[..., ::2])
    with pytest.raises(CrtfxError) as e:
        plan.set_option(99, 1)
    assert e.value.code == _lib.E_INVALID and "option" in str(e.value)
    with pytest.raises(CrtfxError) as e:
        _plan((1, 8), pix, "tff", fields)
    assert e.value.code == _lib.E_INVALID and "h = 1" in str(e.value)
    plan.close()


@pytest.mark.parametrize("fields", model.FIELDS)
@pytest.mark.parametrize("pix", list(DTYPES))
def test_push_in_batches_is_one_run_and_reset_forgets(pix, fields):
    import torch
    size = (9, 24)
    per = 2 if fields == "both" else 1
    src, _ = scene(pix, 7, 9, 24, seed=17)
    x = torch.from_numpy(src).to(_dev())
    plan = _plan(size, pix, "bff", fields)
    whole = plan.run(x)
    staged = torch.empty_like(x[:4])                                           # a slot that is reused: push keeps a copy of its own
    parts = []
    for lo, hi in ((0, 1), (1, 5), (5, 7)):
        staged[:hi - lo].copy_(x[lo:hi])
        parts.append(plan.push(staged[:hi - lo]).clone())
        staged.zero_()
        assert tuple(plan.push(x[:0]).shape) == (0,) + size + (3,)            # n = 0 keeps what it had
    torch.cuda.synchronize()
    assert _same(torch.cat(parts).cpu().numpy(), whole.cpu().numpy()) == 0
    assert _same(whole.cpu().numpy(), model.adaptive(src, None, "bff", fields)) == 0
    again = plan.push(x[:2])                                                   # behind frame 6
    plan.reset()
    fresh = plan.push(x[:2])                                                   # no previous frame: frame 0 is EDGE's
    torch.cuda.synchronize()
    assert _same(again.cpu().numpy(), model.adaptive(src[:2], src[6], "bff", fields)) == 0
    assert _same(fresh.cpu().numpy(), whole[:2 * per].cpu().numpy()) == 0
    assert _same(fresh[:per].cpu().numpy(), dm.deinterlace(src[:1], "edge", "bff", fields)) == 0
    plan.close()


@pytest.mark.parametrize("pix,order,fields", [("u8", "bff", "both"), ("f16", "tff", "both")])
def test_a_full_size_batch(pix, order, fields):
    import torch
    n, size = 3, (480, 720)
    src, prev = scene(pix, n, 480, 720, seed=480)
    plan = _plan(size, pix, order, fields)
    out = plan.run(torch.from_numpy(src).to(_dev()), prev=torch.from_numpy(prev).to(_dev()))
    torch.cuda.synchronize()
    assert plan.plan() == {"adeint": _name(pix, fields, True), "frames": "3"}
    exp, parts = model.adaptive_parts(src, prev, order, fields)
    assert _same(out.cpu().numpy(), exp) == 0 and clamp_classes(parts) == {"weave", "held", "edge"}
    plan.close()
