"""The source probe on the GPU (include/crtfx_probe.h) against tests/probe_model.py: both sample types, both paths, with a previous frame,
without one and with one inside the source batch.  Every comparison is exact: no word may differ."""
import numpy as np
import pytest

from pythoncrt_amd import _lib
from tests import deint_model as dm
from tests import probe_model as model

pytestmark = pytest.mark.gpu

GUARD = 0xA5
# h = 1, 2: no interior row; 3: one; 5 x 7, 13 x 24, 23 x 40: odd sizes, a wave's 8 rows crossed; then the edges of the tile of 32 rows x
# 512 columns (vec) or 64 columns (general), one row and 8 columns to either side
SHAPES = [(1, 1), (1, 8), (2, 8), (3, 8), (5, 7), (8, 16), (13, 24), (23, 40), (31, 504), (32, 512), (33, 520), (33, 56), (31, 64), (32, 72)]
DTYPES = {"u8": np.uint8, "f16": np.float16}
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 255.5, 254.875, 0.125, 0.375, 6e-8, 65504.0, 100.1, -3.0], dtype=np.float16)


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _torch_dtype(pix):
    import torch
    return torch.uint8 if pix == "u8" else torch.float16


def _plan(size, pix, force=False):
    import pythoncrt_amd as pc
    return pc.Probe(_dev(), size, dtype=_torch_dtype(pix), force_general=force)


def noise(pix, n, h, w, seed):
    """n + 1 frames of seeded noise; half frames also carry patterns that cross every rule of the quantiser."""
    f = dm.noise(h, w, n + 1, DTYPES[pix], seed).copy()
    if pix == "f16":
        rng = np.random.default_rng(seed + 1)
        flat = f.reshape(-1)
        pick = rng.integers(0, flat.size, max(1, flat.size // 16))
        flat[pick] = rng.choice(SPECIALS, pick.size)
    return f[1:], f[0]


def _diff(got, exp):
    """The number of differing words, after printing where the first ones are (frame, word, got, expected)."""
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.dtype == np.uint32 and got.shape == exp.shape, (got.dtype, got.shape, exp.shape)
    bad = np.argwhere(got != exp)
    for i, j in bad[:8]:
        print(f"frame {i} word {j}: got {got[i, j]}, expected {exp[i, j]}")
    return len(bad)


def _name(pix, vec):
    return f"k_probe<{pix},{'vec' if vec else 'general'}>"


@pytest.mark.parametrize("force", [False, True], ids=["auto", "forced"])
@pytest.mark.parametrize("pix", list(DTYPES))
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_against_the_model(size, pix, force):
    import torch
    h, w = size
    for n in (1, 2, 3, 5):
        src, prev = noise(pix, n, h, w, seed=h * 1000 + w * 10 + n)
        x, pv = torch.from_numpy(src).to(_dev()), torch.from_numpy(prev).to(_dev())
        plan = _plan(size, pix, force)
        assert plan.words == model.words(h, w)
        for p_np, p_t in ((None, None), (prev, pv), (src[n - 1], x[n - 1])):      # none, given, inside the source batch
            out = plan.run(x, prev=p_t)
            torch.cuda.synchronize()
            assert _diff(out, model.records(src, p_np)) == 0, (size, pix, force, n, p_np is None)
            vec = not force and w % 8 == 0                                        # fresh allocations are aligned
            assert plan.plan() == {"probe": _name(pix, vec), "frames": str(n)}, plan.last_plan()
        plan.close()


@pytest.mark.parametrize("force", [False, True], ids=["vec", "general"])
@pytest.mark.parametrize("pix", list(DTYPES))
def test_constant_and_two_level_contents(pix, force):
    """A constant frame: every lane of every wave holds one bin.  Noise of {0, 1020}: two bins, the widest comb sums.  At a size with several
    tiles either way."""
    import torch
    h, w = 70, 1032 if not force else 136
    rng = np.random.default_rng(5)
    flat = np.full((3, h, w, 3), 37, dtype=DTYPES[pix])
    flat[1] = 255
    two = (rng.integers(0, 2, (3, h, w, 3)) * 255).astype(DTYPES[pix])
    plan = _plan((h, w), pix, force)
    for src in (flat, two):
        x = torch.from_numpy(src).to(_dev())
        out = plan.run(x, prev=x[2])
        torch.cuda.synchronize()
        exp = model.records(src, src[2])
        assert _diff(out, exp) == 0 and plan.plan()["probe"] == _name(pix, not force)
    assert int(exp[0, 16]) + int(exp[0, 16 + 255]) + int(exp[0, 16:272][1:255].sum()) == h * w
    plan.close()


@pytest.mark.parametrize("force", [False, True], ids=["vec", "general"])
def test_every_half_pattern(force):
    """All 65 536 half patterns in a 8 x 2736 frame C and, rolled, in its previous frame P."""
    import torch
    h, w = 8, 2736                                                              # 65 664 samples
    pats = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    frame = lambda roll: np.resize(np.roll(pats, roll), h * w * 3).view(np.float16).reshape(h, w, 3)      # noqa: E731
    src, prev = np.stack([frame(0), frame(40001)]), frame(12345)
    x, pv = torch.from_numpy(src).to(_dev()), torch.from_numpy(prev).to(_dev())
    plan = _plan((h, w), "f16", force)
    out = plan.run(x, prev=pv)
    torch.cuda.synchronize()
    assert plan.plan()["probe"] == _name("f16", not force) and _diff(out, model.records(src, prev)) == 0
    plan.close()


def _guarded(n, frame_bytes, stride_bytes, offset, dtype, align=1):
    """(the guarded uint8 buffer, a [n, frame elements] view of `dtype` into it at byte `offset` behind an `align`-byte boundary, with frame
    stride `stride_bytes`, the view's byte position in the buffer)."""
    import torch
    item = torch.empty((), dtype=dtype).element_size()
    total = 128 + offset + n * stride_bytes + frame_bytes + 64
    total += -total % 8
    buf = torch.full((total,), GUARD, dtype=torch.uint8, device=_dev())
    at = 64 + (-(buf.data_ptr() + 64) % align) + offset
    body = buf[at:at + (n - 1) * stride_bytes + frame_bytes]
    view = body.view(dtype).as_strided((n, frame_bytes // item), (stride_bytes // item, 1))
    assert view.data_ptr() == buf.data_ptr() + at
    return buf, view, at


def _guards_intact(buf, n, frame_bytes, stride_bytes, at):
    b = buf.cpu().numpy().copy()
    for i in range(n):
        b[at + i * stride_bytes:at + i * stride_bytes + frame_bytes] = GUARD
    return bool((b == GUARD).all())


@pytest.mark.parametrize("pix", list(DTYPES))
@pytest.mark.parametrize("size", [(3, 8), (9, 24), (5, 13)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_base_offset_unequal_strides_and_guarded_records(size, pix):
    """Source frames at every byte offset (0..3; 0, 2 for halves) with a stride a few bytes longer than a frame, the previous frame at every
    offset too, records 8 or 24 bytes further apart than a record: the words are the model's, the path is the one the header's conditions
    give, no byte outside the records changes, the source is untouched, and a second run into the same buffer gives the same words."""
    import torch
    h, w = size
    dt, item = _torch_dtype(pix), (1 if pix == "u8" else 2)
    fb, words, n = h * w * 3 * item, model.words(h, w), 3
    src_np, prev = noise(pix, n, h, w, seed=7 * h + w)
    exp = model.records(src_np, prev)
    offsets = range(4) if pix == "u8" else (0, 2)
    plan = _plan(size, pix)
    seen = set()
    for s_off in offsets:
        for p_off in offsets:
            for s_gap, r_gap in ((0, 8), (4, 24), (item, 0), (8 + item, 8)):
                sb, s, s_at = _guarded(n, fb, fb + s_gap, s_off, dt, align=4)
                pb, p, p_at = _guarded(1, fb, fb, p_off, dt, align=4)
                rb, r, r_at = _guarded(n, 4 * words, 4 * words + r_gap, 0, torch.uint32, align=8)
                s.copy_(torch.from_numpy(src_np.reshape(n, -1)).to(_dev()))
                p.copy_(torch.from_numpy(prev.reshape(1, -1)).to(_dev()))
                s4 = s.as_strided((n, h, w, 3), (s.stride(0), w * 3, 3, 1))
                p3 = p[0].view(h, w, 3)
                assert s4.data_ptr() % 4 == s_off and p3.data_ptr() % 4 == p_off and r.data_ptr() % 8 == 0
                for _ in range(2):                                              # the same buffer run twice
                    plan.run(s4, prev=p3, out=r)
                    torch.cuda.synchronize()
                    got = rb.cpu().numpy()[r_at:r_at + n * (4 * words + r_gap)].reshape(n, -1)[:, :4 * words]      # read through the guarded bytes
                    assert _diff(np.ascontiguousarray(got).view(np.uint32), exp) == 0, (s_off, p_off, s_gap, r_gap)
                vec = w % 8 == 0 and s_off == 0 and p_off == 0 and (fb + s_gap) % 4 == 0
                seen.add(vec)
                assert plan.plan()["probe"] == _name(pix, vec), (s_off, p_off, s_gap, plan.last_plan())
                assert _guards_intact(rb, n, 4 * words, 4 * words + r_gap, r_at)
                assert _guards_intact(sb, n, fb, fb + s_gap, s_at) and _guards_intact(pb, 1, fb, fb, p_at)
                assert np.array_equal(dm.bits(s4.cpu().numpy()), dm.bits(src_np))
    plan.close()
    assert seen == ({False} if w % 8 else {True, False})


@pytest.mark.parametrize("pix", list(DTYPES))
def test_no_frames_a_long_batch_and_the_call_forms(pix):
    import torch
    size = (3, 8)
    plan = _plan(size, pix)
    src_np, prev = noise(pix, 65, 3, 8, seed=65)
    x, pv = torch.from_numpy(src_np).to(_dev()), torch.from_numpy(prev).to(_dev())
    out = plan.run(x, prev=pv)                                                 # 65 frames of 3 x 8 in one grid
    torch.cuda.synchronize()
    assert plan.plan() == {"probe": _name(pix, True), "frames": "65"} and _diff(out, model.records(src_np, prev)) == 0
    assert _diff(plan(x), model.records(src_np)) == 0                          # plan(x) == plan.run(x): no previous frame
    empty = plan.run(x[:0], prev=pv)
    assert tuple(empty.shape) == (0, plan.words) and empty.dtype == torch.uint32
    keep = out.cpu().numpy().copy()
    assert plan.run(x[:0], out=out[:0]).data_ptr() == out[:0].data_ptr()       # n = 0: `out` comes back untouched
    st = torch.cuda.current_stream().cuda_stream
    run = plan.lib.crtfx_probe_run
    assert run(plan._plan, pv.data_ptr(), x.data_ptr(), 0, out.data_ptr(), 0, 0, st) == _lib.OK
    assert run(plan._plan, None, None, 0, None, 0, 0, st) == _lib.OK
    torch.cuda.synchronize()
    assert _diff(out, keep) == 0 and plan.plan()["frames"] == "0"
    plan.force_general = True                                                  # switches the plan string and not the words
    assert plan.force_general and plan.plan()["probe"] == _name(pix, False)
    forced = plan.run(x, prev=pv)
    torch.cuda.synchronize()
    assert plan.plan() == {"probe": _name(pix, False), "frames": "65"} and _diff(forced, keep) == 0
    plan.force_general = False
    assert plan.plan()["probe"] == _name(pix, True)
    plan.close()


@pytest.mark.parametrize("force", [False, True], ids=["vec", "general"])
def test_a_batch_past_one_launch_group(force):
    """32 769 frames of 2 x 8 uint8: the last frame is a launch of its own and takes frame 32 767 as its previous frame.  h = 2 has no
    interior row, so what shows the previous frame is the flag; every record against the model's, computed at once."""
    import torch
    n, size = 32769, (2, 8)
    rng = np.random.default_rng(32769)
    src = rng.integers(0, 256, (n,) + size + (3,), dtype=np.uint8)
    x = torch.from_numpy(src).to(_dev())
    plan = _plan(size, "u8", force)
    out = plan.run(x)
    torch.cuda.synchronize()
    assert plan.plan() == {"probe": _name("u8", not force), "frames": str(n)}
    got = out.cpu().numpy()
    Y = model.luma(src)
    exp = np.zeros((n, model.words(2, 8)), dtype=np.int64)
    exp[1:, 0] = 1
    c = model.codes(src).reshape(n, -1, 3)
    exp[:, 1:4], exp[:, 4:7], exp[:, 8] = c.min(axis=1), c.max(axis=1), Y.sum(axis=(1, 2))
    np.add.at(exp, (np.repeat(np.arange(n), 16), 16 + (Y >> 2).reshape(-1)), 1)
    exp[:, 272:274], exp[:, 274:282] = Y.sum(axis=2), Y.sum(axis=1)
    assert _diff(got, exp.astype(np.uint32)) == 0 and got[32768, 0] == 1
    for i in (0, 1, 32767, 32768):
        assert np.array_equal(got[i], model.record(src[i], src[i - 1] if i else None)), i
    plan.close()


@pytest.mark.parametrize("pix", list(DTYPES))
def test_push_in_batches_is_one_run_and_reset_forgets(pix):
    import torch
    size = (9, 24)
    src, _ = noise(pix, 7, 9, 24, seed=17)
    x = torch.from_numpy(src).to(_dev())
    plan = _plan(size, pix)
    whole = plan.run(x)
    staged = torch.empty_like(x[:4])                                           # a slot that is reused: push keeps a copy of its own
    parts = []
    for lo, hi in ((0, 1), (1, 5), (5, 7)):
        staged[:hi - lo].copy_(x[lo:hi])
        parts.append(plan.push(staged[:hi - lo]).cpu().numpy())
        staged.zero_()
        assert tuple(plan.push(x[:0]).shape) == (0, plan.words)                # n = 0 keeps what it had
    torch.cuda.synchronize()
    assert _diff(np.concatenate(parts), whole.cpu().numpy()) == 0 and _diff(whole, model.records(src)) == 0
    again = plan.push(x[:2])                                                   # behind frame 6
    plan.reset()
    fresh = plan.push(x[:2])                                                   # no previous frame
    torch.cuda.synchronize()
    assert _diff(again, model.records(src[:2], src[6])) == 0 and _diff(fresh, model.records(src[:2])) == 0
    assert int(again[0, 0]) == 1 and int(fresh[0, 0]) == 0
    plan.close()


@pytest.mark.parametrize("pix", list(DTYPES))
def test_run_refusals(pix):
    """What the sibling families refuse, a record base or stride that is not a multiple of 8, and records that overlap the source or
    prev_frame; no refused call writes anything."""
    import torch
    from pythoncrt_amd._lib import CrtfxError
    size, n = (3, 8), 2
    plan = _plan(size, pix)
    fb, rb = 72 * (1 if pix == "u8" else 2), 4 * model.words(3, 8)
    src = torch.zeros(n * fb + 16, dtype=torch.uint8, device=_dev())
    dst = torch.zeros(n * rb + 64, dtype=torch.uint8, device=_dev())
    prv = torch.zeros(fb + 16, dtype=torch.uint8, device=_dev())
    run, err = plan.lib.crtfx_probe_run, plan.lib.crtfx_probe_last_error
    st = torch.cuda.current_stream().cuda_stream
    sp, dp, pp = src.data_ptr(), dst.data_ptr(), prv.data_ptr()
    assert dp % 8 == 0
    if pix == "f16":
        assert run(plan._plan, pp, sp + 1, fb, dp, rb, 1, st) == _lib.E_INVALID and b"even" in err(plan._plan)
        assert run(plan._plan, pp, sp, fb + 1, dp, rb, n, st) == _lib.E_INVALID and b"even" in err(plan._plan)
        assert run(plan._plan, pp + 1, sp, fb, dp, rb, n, st) == _lib.E_INVALID and b"even prev_frame" in err(plan._plan)
    for off in (1, 2, 4, 7):
        assert run(plan._plan, pp, sp, fb, dp + off, rb, n, st) == _lib.E_INVALID and b"multiples of 8" in err(plan._plan), off
        assert run(plan._plan, pp, sp, fb, dp, rb + off, n, st) == _lib.E_INVALID and b"multiples of 8" in err(plan._plan), off
    assert run(plan._plan, pp, sp, fb - 2, dp, rb, n, st) == _lib.E_INVALID and b"strides" in err(plan._plan)
    assert run(plan._plan, pp, sp, fb, dp, rb - 8, n, st) == _lib.E_INVALID and b"strides" in err(plan._plan)
    assert run(plan._plan, pp, None, fb, dp, rb, 1, st) == _lib.E_INVALID and b"null" in err(plan._plan)
    assert run(plan._plan, pp, sp, fb, None, rb, 1, st) == _lib.E_INVALID
    assert run(plan._plan, pp, sp, fb, dp, rb, -1, st) == _lib.E_INVALID and b"n = -1" in err(plan._plan)
    both = torch.zeros(n * (fb + rb) + fb + 64, dtype=torch.uint8, device=_dev())
    bp = both.data_ptr()
    at = -(-(n * fb) // 8) * 8                                                   # the first multiple of 8 behind the source range
    for s_at, d_at in ((0, 0), (8, 0), (0, at - 8)):
        assert run(plan._plan, pp, bp + s_at, fb, bp + d_at, rb, n, st) == _lib.E_INVALID and b"source and destination overlap" in err(plan._plan), (s_at, d_at)
    for p_at in (dp, dp + n * rb - 2, dp + rb, dp - fb + 2):
        assert run(plan._plan, p_at, sp, fb, dp, rb, n, st) == _lib.E_INVALID and b"prev_frame and destination overlap" in err(plan._plan), p_at - dp
    assert run(plan._plan, bp, bp, fb, bp + at, rb, n, st) == _lib.OK          # touching ranges do not overlap; prev inside the source range
    torch.cuda.synchronize()
    assert int(dst.sum()) == 0 and int(src.sum()) == 0 and int(prv.sum()) == 0
    x = torch.zeros((n,) + size + (3,), dtype=_torch_dtype(pix), device=_dev())
    with pytest.raises(CrtfxError) as e:
        plan.run(x.to(torch.float32))                                           # a wrong dtype
    assert e.value.code == _lib.E_UNSUPPORTED
    with pytest.raises(ValueError, match="frames must be"):
        plan.run(x[:, :2])
    with pytest.raises(ValueError, match="out must be uint32"):
        plan.run(x, out=torch.empty((n, plan.words), dtype=torch.int32, device=_dev()))
    with pytest.raises(ValueError, match="out must be uint32"):
        plan.run(x, out=torch.empty((n, plan.words + 2), dtype=torch.uint32, device=_dev()))
    for bad in (x, x[0, :2], x[0].cpu(), x[0].to(torch.float32)):
        with pytest.raises(ValueError, match="prev must be"):
            plan.run(x, prev=bad)
    with pytest.raises(CrtfxError) as e:
        plan.set_option(99, 1)
    assert e.value.code == _lib.E_INVALID and "option" in str(e.value)
    with pytest.raises(CrtfxError) as e:
        _plan((0, 8), pix)
    assert e.value.code == _lib.E_INVALID and "h = 0" in str(e.value)
    one = _plan((1, 8), pix)                                                    # h = 1 is allowed
    assert one.words == model.words(1, 8)
    one.close()
    plan.close()


@pytest.mark.parametrize("size,pix,force", [((480, 720), "u8", False), ((480, 720), "f16", False), ((480, 720), "u8", True),
                                            ((1080, 1920), "u8", False), ((1080, 1920), "f16", False)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_a_full_size_batch_of_8(size, pix, force):
    import torch
    h, w = size
    rng = np.random.default_rng(h)
    base = rng.integers(0, 256, (9, h, w, 3), dtype=np.uint8)
    base[:, : h // 8] //= 16                                                    # a dark band on top: bins that many lanes share
    src = base if pix == "u8" else base.astype(np.float16)
    plan = _plan(size, pix, force)
    x = torch.from_numpy(src).to(_dev())
    out = plan.run(x[1:], prev=x[0])
    torch.cuda.synchronize()
    assert plan.plan() == {"probe": _name(pix, not force), "frames": "8"}
    assert _diff(out, model.records(base[1:], base[0])) == 0                    # half(u) has the code 4 u: one model for both
    plan.close()
