"""The 3D LUT stage on the GPU (include/crtfx_lut3d.h) against tests/lut3d_model.py: both sample types, the cube in LDS and in device
memory, four pixels per lane and one.  Every comparison is exact: no element may differ."""

import ctypes

import numpy as np
import pytest

from pythoncrt_amd import _lib
from pythoncrt_amd.cube import Cube
from tests import lut3d_model as model

pytestmark = pytest.mark.gpu

GUARD = 0xA5
SHAPES = [(1, 1), (1, 3), (2, 5), (3, 4), (5, 7), (7, 9), (23, 40)]    # whole chunks of 4 pixels, tails of 1, 2 and 3, frames smaller than a chunk
SIZES = [2, 3, 17, 33, 34, 35, 65]                                     # 34: the last cube the lds path holds; 35: the first that is global only
DTYPES = ["uint8", "float16"]
PATHS = [(False, False), (False, True), (True, False), (True, True)]   # (force_global, force_general)


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _cube(n, seed=0):
    """A random cube whose quantised table is model.random_table(n, seed): quarter codes / 1020 are exact enough to round back."""
    t = model.random_table(n, seed)
    c = Cube(n, t.astype(np.float64) / 1020.0)
    assert np.array_equal(c.quantise(), t)
    return c, t


def _plan(size, cube, dtype, force_global=False, force_general=False):
    import torch
    import pythoncrt_amd as pc
    plan = pc.Lut3D(_dev(), size, cube, dtype=getattr(torch, dtype), force_general=force_general)
    if force_global:
        plan.force_global = True
    return plan


def _frames(dtype, shape, seed=0):
    n_px = int(np.prod(shape[:-1]))
    return model.pixels(np.dtype(dtype).type, n_px, seed=seed).reshape(shape)


def _same(got, exp):
    """Bit for bit: halves are compared as their patterns."""
    assert got.dtype == exp.dtype and got.shape == exp.shape
    if got.dtype == np.float16:
        got, exp = got.view(np.uint16), exp.view(np.uint16)
    return int((got != exp).sum())


def _vec_expected(src, dst, n, force=False):
    """The header's conditions, from the tensors' own addresses and strides."""
    if force or (src.data_ptr() | dst.data_ptr()) & 3:
        return False
    return n <= 1 or not ((src.stride(0) * src.element_size() | dst.stride(0) * dst.element_size()) & 3)


def _name(dtype, n_cube, force_global, vec):
    table = "lds" if n_cube <= 34 and not force_global else "global"
    return f"k_lut3d<{'u8' if dtype == 'uint8' else 'half'},{table},{'vec' if vec else 'general'}>"


def _plan_dict(dtype, n_cube, force_global, vec, frames):
    lds = 4 * n_cube ** 3 if n_cube <= 34 and not force_global else 0
    return {"lut3d": _name(dtype, n_cube, force_global, vec), "n": str(n_cube), "lds": str(lds), "frames": str(frames)}


@pytest.mark.parametrize("n_cube", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_shapes_paths_and_cubes_against_the_model(dtype, n_cube):
    """Every shape x the four paths x a random cube and the identity cube (swapped in on the live plan), one frame and three."""
    import torch
    cube, table = _cube(n_cube, seed=1)
    ident = Cube.identity(n_cube)
    for size in SHAPES:
        srcs = {n: _frames(dtype, (n,) + size + (3,), seed=n_cube + n) for n in (1, 3)}
        want = {n: model.apply(s, table) for n, s in srcs.items()}
        plan = _plan(size, cube, dtype)
        for force_global, force_general in PATHS:
            plan.force_global, plan.force_general = force_global, force_general
            assert plan.plan() == _plan_dict(dtype, n_cube, force_global, not force_general, 0)
            for n, src in srcs.items():
                x = torch.from_numpy(src).to(_dev())
                out = plan.run(x)
                torch.cuda.synchronize()
                assert _same(out.cpu().numpy(), want[n]) == 0, (size, dtype, n_cube, force_global, force_general, n)
                vec = _vec_expected(x, out, n, force_general)
                assert plan.plan() == _plan_dict(dtype, n_cube, force_global, vec, n), plan.last_plan()
                if not force_general and n == 1:
                    assert vec                                                  # fresh allocations are aligned
        # the identity cube on the live plan: quarter codes come back (uint8 codes unchanged; halves as the code of their quantiser)
        plan.set_cube(ident)
        for force_global, force_general in PATHS:
            plan.force_global, plan.force_general = force_global, force_general
            x = torch.from_numpy(srcs[3]).to(_dev())
            out = plan.run(x).cpu().numpy()
            assert _same(out, model.apply(srcs[3], model.identity_table(n_cube))) == 0
            if dtype == "uint8":
                assert np.array_equal(out, srcs[3])
        plan.close()


@pytest.mark.parametrize("n_cube", [33, 35])
def test_every_half_pattern_in_one_channel(n_cube):
    """All 65 536 half patterns in channel c of frame c, random quarter codes beside them, on both walks."""
    import torch
    rng = np.random.default_rng(n_cube)
    halves = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    frames = (rng.integers(0, 1021, (3, 65536, 3)) / 4.0).astype(np.float16)
    for c in range(3):
        frames[c, :, c] = np.roll(halves, 1 + 7 * c)                            # off the chunk grid
    frames = frames.reshape(3, 64, 1024, 3)
    cube, table = _cube(n_cube, seed=2)
    want = model.apply(frames, table)
    for force_general in (False, True):
        plan = _plan((64, 1024), cube, "float16", force_general=force_general)
        out = plan.run(torch.from_numpy(frames).to(_dev()))
        torch.cuda.synchronize()
        assert plan.plan()["lut3d"] == _name("float16", n_cube, False, not force_general)
        assert _same(out.cpu().numpy(), want) == 0
        plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_grey_pixels_and_pixels_at_the_top_edge(dtype):
    """Grey pixels (the three fractions are equal: every tie at once) and pixels with one, two and three channels at S, on all four paths."""
    import torch
    top = 255 if dtype == "uint8" else 1020
    g = np.arange(top + 1)
    grey = np.stack([g, g, g], -1)
    edges = np.array([[(m >> c & 1) * top or (37 * (c + 1) * m) % top for c in range(3)] for m in range(1, 8)] * 9)
    codes = np.concatenate([grey, edges])
    codes = np.concatenate([codes, codes[:(-len(codes)) % 11]]).reshape(1, -1, 11, 3)
    frames = codes.astype(np.uint8) if dtype == "uint8" else (codes / 4.0).astype(np.float16)
    for n_cube in (17, 35):
        cube, table = _cube(n_cube, seed=3)
        want = model.apply(frames, table)
        plan = _plan(frames.shape[1:3], cube, dtype)
        for force_global, force_general in PATHS:
            plan.force_global, plan.force_general = force_global, force_general
            out = plan.run(torch.from_numpy(frames).to(_dev())).cpu().numpy()
            assert _same(out, want) == 0, (dtype, n_cube, force_global, force_general)
        plan.close()


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


@pytest.mark.parametrize("force_global", [False, True], ids=["lds", "global"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", [(3, 4), (5, 7), (1, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_base_offset_inside_guards(size, dtype, force_global):
    """uint8 frames at byte offsets 0..3, half frames at 0 and 2, on either side independently, three frames with strides a few bytes
    longer than a frame: the bytes are the model's, the walk is the one the header's conditions give, and no byte outside the frames
    changes."""
    import torch
    h, w = size
    tdt = getattr(torch, dtype)
    item = 1 if dtype == "uint8" else 2
    fb = h * w * 3 * item
    cube, table = _cube(17, seed=4)
    plan = _plan(size, cube, dtype, force_global=force_global)
    offsets = range(4) if dtype == "uint8" else (0, 2)
    gaps = ((0, 0), (4, 8), (3, 3), (1, 2)) if dtype == "uint8" else ((0, 0), (4, 8), (2, 6), (6, 2))
    seen, n = set(), 3
    for s_off in offsets:
        for d_off in offsets:
            for s_gap, d_gap in gaps:
                src_np = _frames(dtype, (n,) + size + (3,), seed=s_off * 16 + d_off * 4 + s_gap)
                sb, s = _guarded(n, fb, fb + s_gap, s_off, tdt)
                db, d = _guarded(n, fb, fb + d_gap, d_off, tdt)
                s.copy_(torch.from_numpy(src_np.reshape(n, -1)).to(_dev()))
                s4 = s.as_strided((n, h, w, 3), (s.stride(0), w * 3, 3, 1))
                d4 = d.as_strided((n, h, w, 3), (d.stride(0), w * 3, 3, 1))
                plan.run(s4, out=d4)
                torch.cuda.synchronize()
                vec = _vec_expected(s4, d4, n)
                seen.add(vec)
                assert plan.plan()["lut3d"] == _name(dtype, 17, force_global, vec), (s_off, d_off, s_gap, d_gap, plan.last_plan())
                assert _same(d4.cpu().numpy(), model.apply(src_np, table)) == 0, (s_off, d_off, s_gap, d_gap)
                assert _guards_intact(db, n, fb, fb + d_gap, d_off) and _guards_intact(sb, n, fb, fb + s_gap, s_off)
    assert seen == {True, False}
    plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_batches_with_unequal_strides_and_slices(dtype):
    """Slices of larger tensors: the source's batch stride and the destination's differ, and both exceed a frame."""
    import torch
    size, n = (7, 9), 4
    src_np = _frames(dtype, (n, 2) + size + (3,), seed=12)
    big_src = torch.from_numpy(src_np).to(_dev())
    big_dst = torch.zeros((n, 3) + size + (3,), dtype=big_src.dtype, device=_dev())
    cube, table = _cube(33, seed=5)
    plan = _plan(size, cube, dtype)
    out = plan.run(big_src[:, 1], out=big_dst[:, 2])
    torch.cuda.synchronize()
    vec = _vec_expected(big_src[:, 1], big_dst[:, 2], n)
    assert out.data_ptr() == big_dst[:, 2].data_ptr() and plan.plan() == _plan_dict(dtype, 33, False, vec, n)
    assert _same(big_dst[:, 2].cpu().numpy(), model.apply(src_np[:, 1], table)) == 0
    assert int(big_dst[:, :2].view(torch.uint8).sum()) == 0                     # the frames between: untouched
    with pytest.raises(ValueError, match="contiguous"):
        plan.run(torch.zeros((n,) + size + (6,), dtype=big_src.dtype, device=_dev())[..., ::2])      # the right shape, frames with holes
    plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_frames_a_long_batch_and_the_call_forms(dtype):
    import torch
    size = (3, 4)
    cube, table = _cube(33, seed=6)
    plan = _plan(size, cube, dtype)
    src_np = _frames(dtype, (65,) + size + (3,), seed=65)
    x = torch.from_numpy(src_np).to(_dev())
    out = plan.run(x)                                                          # 65 frames of 3 x 4 in one launch
    torch.cuda.synchronize()
    assert plan.plan() == _plan_dict(dtype, 33, False, True, 65)
    assert _same(out.cpu().numpy(), model.apply(src_np, table)) == 0
    assert torch.equal(plan(x).view(torch.uint8), out.view(torch.uint8))       # plan(x) == plan.run(x)
    empty = plan.run(x[:0])
    assert tuple(empty.shape) == (0,) + size + (3,) and empty.dtype == out.dtype
    # n = 0 through the C entry point: nothing runs, nothing is written, nothing is asked of the pointers
    keep = out.clone()
    st = torch.cuda.current_stream().cuda_stream
    assert plan.lib.crtfx_lut3d_run(plan._plan, x.data_ptr(), 0, out.data_ptr(), 0, 0, st) == _lib.OK
    assert plan.lib.crtfx_lut3d_run(plan._plan, None, 0, None, 0, 0, st) == _lib.OK
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.uint8), keep.view(torch.uint8)) and plan.plan()["frames"] == "0"
    # the switches change the plan string and not the bytes
    for force_global, force_general in PATHS[1:]:
        plan.force_global, plan.force_general = force_global, force_general
        assert (plan.force_global, plan.force_general) == (force_global, force_general)
        forced = plan.run(x)
        torch.cuda.synchronize()
        assert plan.plan() == _plan_dict(dtype, 33, force_global, not force_general, 65)
        assert torch.equal(forced.view(torch.uint8), out.view(torch.uint8))
    plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_set_cube_on_a_live_plan_gives_the_bits_of_a_fresh_plan(dtype):
    import torch
    from pythoncrt_amd._lib import CrtfxError
    size = (23, 40)
    src_np = _frames(dtype, (2,) + size + (3,), seed=8)
    x = torch.from_numpy(src_np).to(_dev())
    for n_cube in (33, 35):
        a, ta = _cube(n_cube, seed=10)
        b, tb = _cube(n_cube, seed=11)
        live = _plan(size, a, dtype)
        first = live.run(x).cpu().numpy()
        live.set_cube(b)
        assert live.cube is b
        swapped = live.run(x).cpu().numpy()
        fresh = _plan(size, b, dtype)
        assert _same(first, model.apply(src_np, ta)) == 0 and _same(swapped, model.apply(src_np, tb)) == 0
        assert _same(swapped, fresh.run(x).cpu().numpy()) == 0 and _same(first, swapped) > 0
        # another N, and an entry above 1020, are refused and the plan keeps its cube
        with pytest.raises(CrtfxError, match="differs from the plan's N") as e:
            live.set_cube(Cube.identity(n_cube - 1))
        assert e.value.code == _lib.E_INVALID and live.cube is b
        bad = tb.copy()
        bad[1, 0, 2, 1] = 1021
        rc = live.lib.crtfx_lut3d_set_table(live._plan, n_cube, np.ascontiguousarray(bad).ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)))
        assert rc == _lib.E_INVALID and b"= 1021 above 1020" in live.lib.crtfx_lut3d_last_error(live._plan)
        assert live.lib.crtfx_lut3d_set_table(live._plan, n_cube, None) == _lib.E_INVALID
        assert _same(live.run(x).cpu().numpy(), swapped) == 0
        live.close()
        fresh.close()


@pytest.mark.parametrize("force_general", [False, True], ids=["vec", "general"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_lds_plans_of_different_sizes_live_side_by_side(dtype, force_general):
    """The dynamic-LDS limit belongs to the kernel function, not to a plan: an N = 34 plan (157 216 bytes) still runs after plans of
    smaller cubes above 64 KiB (N = 26..33) and below it (N = 17) were created for the same sample type, and each plan gives its own
    cube's bits whatever the order they run in."""
    import torch
    size = (7, 12)                                                             # a frame's bytes are a multiple of 4: the vec walk takes a batch
    src_np = _frames(dtype, (3,) + size + (3,), seed=34)
    x = torch.from_numpy(src_np).to(_dev())
    plans = []
    for n_cube in (34, 26, 32, 33, 17):
        cube, table = _cube(n_cube, seed=20 + n_cube)
        plans.append((n_cube, _plan(size, cube, dtype, force_general=force_general), model.apply(src_np, table)))
        for m, plan, want in plans:                                            # every plan live so far, the first one first
            out = plan.run(x)
            torch.cuda.synchronize()
            assert plan.plan() == _plan_dict(dtype, m, False, _vec_expected(x, out, 3, force_general), 3), (n_cube, plan.last_plan())
            assert _same(out.cpu().numpy(), want) == 0, (n_cube, m)
    for _, plan, _ in plans:
        plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_run_refusals(dtype):
    """Odd half bases and strides, overlapping ranges, short strides, null pointers, n < 0 and wrong tensors are refused, and no refused call
    writes anything."""
    import torch
    from pythoncrt_amd._lib import CrtfxError
    size, n = (3, 4), 2
    plan = _plan(size, Cube.identity(5), dtype)
    fb = 36 * (1 if dtype == "uint8" else 2)
    src = torch.zeros(n * fb + 16, dtype=torch.uint8, device=_dev())
    dst = torch.zeros(n * fb + 16, dtype=torch.uint8, device=_dev())
    run, err = plan.lib.crtfx_lut3d_run, plan.lib.crtfx_lut3d_last_error
    st = torch.cuda.current_stream().cuda_stream
    sp, dp = src.data_ptr(), dst.data_ptr()
    if dtype == "float16":
        assert run(plan._plan, sp + 1, fb, dp, fb, 1, st) == _lib.E_INVALID and b"even" in err(plan._plan)
        assert run(plan._plan, sp, fb, dp + 1, fb, 1, st) == _lib.E_INVALID and b"even" in err(plan._plan)
        assert run(plan._plan, sp, fb + 1, dp, fb + 2, n, st) == _lib.E_INVALID and b"even" in err(plan._plan)      # an odd stride
        assert run(plan._plan, sp, fb + 2, dp, fb + 3, n, st) == _lib.E_INVALID and b"even" in err(plan._plan)
    assert run(plan._plan, sp, fb - 2, dp, fb, n, st) == _lib.E_INVALID and b"strides" in err(plan._plan)
    assert run(plan._plan, sp, fb, dp, fb - 2, n, st) == _lib.E_INVALID and b"strides" in err(plan._plan)
    assert run(plan._plan, None, fb, dp, fb, 1, st) == _lib.E_INVALID and b"null" in err(plan._plan)
    assert run(plan._plan, sp, fb, None, fb, 1, st) == _lib.E_INVALID
    assert run(plan._plan, sp, fb, dp, fb, -1, st) == _lib.E_INVALID and b"n = -1" in err(plan._plan)
    # overlap: the destination inside the source's range, the source's last bytes on the destination's first, and the same buffer
    both = torch.zeros(2 * n * fb + 8, dtype=torch.uint8, device=_dev())
    bp = both.data_ptr()
    for s_at, d_at in ((0, 0), (0, n * fb - 2), (n * fb - 2, 0), (0, fb)):
        assert run(plan._plan, bp + s_at, fb, bp + d_at, fb, n, st) == _lib.E_INVALID and b"overlap" in err(plan._plan), (s_at, d_at)
    assert run(plan._plan, bp, fb, bp + n * fb, fb, n, st) == _lib.OK         # touching ranges do not overlap
    torch.cuda.synchronize()
    assert int(dst.sum()) == 0 and int(src.sum()) == 0
    x = torch.zeros((n,) + size + (3,), dtype=getattr(torch, dtype), device=_dev())
    for wrong in (torch.float32, torch.float16 if dtype == "uint8" else torch.uint8):
        with pytest.raises(CrtfxError) as e:
            plan.run(x.to(wrong))
        assert e.value.code == _lib.E_UNSUPPORTED
    with pytest.raises(ValueError, match="frames must be"):
        plan.run(x[:, :2])
    with pytest.raises(ValueError, match="out must be"):
        plan.run(x, out=torch.empty((n,) + size + (3,), dtype=torch.float32, device=_dev()))
    with pytest.raises(CrtfxError, match="overlap"):
        plan.run(x, out=x)
    for option, value in ((99, 1), (_lib.LUT3D_OPT_FORCE_GLOBAL, 2), (_lib.LUT3D_OPT_FORCE_GENERAL, -1)):
        with pytest.raises(CrtfxError) as e:
            plan.set_option(option, value)
        assert e.value.code == _lib.E_INVALID
    plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_1080p_batch(dtype):
    import torch
    size, n = (1080, 1920), 2
    rng = np.random.default_rng(1080)
    one = rng.integers(0, 256, size + (3,), dtype=np.uint8) if dtype == "uint8" else \
        (rng.integers(-8, 1040, size + (3,), dtype=np.int16) / np.float32(4.0)).astype(np.float16)
    src_np = np.stack([one, one[::-1, ::-1]])                                  # the operation is pointwise: the second frame's pixels are the first's, reversed
    cube, table = _cube(33, seed=7)
    want = model.apply(one, table)
    plan = _plan(size, cube, dtype)
    out = plan.run(torch.from_numpy(src_np).to(_dev()))
    torch.cuda.synchronize()
    assert plan.plan() == _plan_dict(dtype, 33, False, True, n)
    assert _same(out.cpu().numpy(), np.stack([want, want[::-1, ::-1]])) == 0
    plan.close()
