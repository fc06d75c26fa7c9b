"""What the six frame plans take from their shared base (pythoncrt_amd/_stage.py: Handle, FramePlan) and from the one host skeleton of
their C side (csrc/crtfx_frame_host.h), on the GPU — the counterpart of test_resize_api_gpu.py.  Seven plans: Canvas on uint8 and on
float16, Widen, Narrow("ordered"), Deinterlace("edge", fields="both") on uint8, AdaptiveDeinterlace(fields="both") on float16, Lut3D with a
2 x 2 x 2 cube on uint8.  Calling a plan is run(), last_plan() is plan() unparsed, force_general is a property that set_option moves and
the plan string follows, a batch that is a slice of a wider tensor on both sides gives the frames of a packed one and writes nothing
between them, n == 0 is answered with OK and frames=0 and touches nothing, and a run of 32769 frames crosses the group boundary of the
shared loop.  Outputs are compared with the exact host models (canvas_model, depth_model, deint_model, adeint_model, lut3d_model):
equality, no tolerance."""
import numpy as np
import pytest

from pythoncrt_amd import _lib
from tests import adeint_model, canvas_model, deint_model, depth_model, lut3d_model

pytestmark = pytest.mark.gpu

N = 3
SHAPES = [(3, 5), (2, 8)]                              # an odd width: the general path wherever vec_fits looks at the width; w & 7 == 0: vec
GROUP = 32768                                          # source frames per launch (grid.z)
FILL = (7, 100, 250)
CASES = ["canvas-u8", "canvas-half", "widen", "narrow", "deint", "adeint", "lut3d"]
FAMILY = {"canvas-u8": "canvas", "canvas-half": "canvas", "widen": "depth", "narrow": "depth", "deint": "deint", "adeint": "adeint", "lut3d": "lut3d"}
OPTIONS = {"canvas": "CANVAS_OPT_FORCE_GENERAL", "depth": "DEPTH_OPT_FORCE_GENERAL", "deint": "DEINT_OPT_FORCE_GENERAL",
           "adeint": "ADEINT_OPT_FORCE_GENERAL", "lut3d": "LUT3D_OPT_FORCE_GENERAL"}
HALF_IN = ("canvas-half", "narrow", "adeint")          # the plans that take float16 frames
FRAMES_OUT = {"deint": 2, "adeint": 2}                 # fields="both"
LUT_N = 2


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _canvas_dst(size):
    """The source placed at (1, 2) of a frame one row and four columns larger: bars on three sides, and whole dwords per frame."""
    return (size[0] + 1, size[1] + 4)


def _make(case, size):
    import torch
    import pythoncrt_amd as pc
    from pythoncrt_amd.cube import Cube
    if case.startswith("canvas"):
        return pc.Canvas(_dev(), size, _canvas_dst(size), at=(1, 2), fill=FILL, dtype=torch.uint8 if case == "canvas-u8" else torch.float16)
    if case == "widen":
        return pc.Widen(_dev(), size)
    if case == "narrow":
        return pc.Narrow(_dev(), size, dither="ordered")
    if case == "deint":
        return pc.Deinterlace(_dev(), size, method="edge", fields="both")
    if case == "adeint":
        return pc.AdaptiveDeinterlace(_dev(), size, fields="both", dtype=torch.float16)
    table = lut3d_model.random_table(LUT_N)
    cube = Cube(LUT_N, table.astype(np.float64) / 1020.0)
    assert np.array_equal(cube.quantise(), table)
    return pc.Lut3D(_dev(), size, cube)


def _model(case, frames):
    """The host model of the plan `_make` builds."""
    size = frames.shape[1:3]
    if case.startswith("canvas"):
        return canvas_model.canvas(frames, _canvas_dst(size), at=(1, 2), fill=np.array(FILL, dtype=frames.dtype))
    if case == "widen":
        return depth_model.widen(frames)
    if case == "narrow":
        return depth_model.narrow(frames, "ordered")
    if case == "deint":
        return deint_model.deinterlace(frames, "edge", "tff", "both")
    if case == "adeint":
        return adeint_model.adaptive(frames, None, "tff", "both")
    return lut3d_model.apply(frames, lut3d_model.random_table(LUT_N))


def _vec(case, size, src=None, dst=None):
    """Whether frames of `size` take the vec kernel, from what each header states for its vec_fits: the size alone for a plan that has not
    run (or ran no frame); with the batch `src` -> `dst`, also dword-aligned bases and, between frames, strides of whole dwords (the
    canvas looks at the destination only)."""
    if case.startswith("canvas"):
        h, w = _canvas_dst(size)
        fits = h * w * 3 * (1 if case == "canvas-u8" else 2) % 4 == 0
    else:
        fits = case in ("widen", "lut3d") or size[1] % 8 == 0
    for t in () if src is None else (dst,) if case.startswith("canvas") else (src, dst):
        fits = fits and t.data_ptr() % 4 == 0 and (t.shape[0] <= 1 or t.stride(0) * t.element_size() % 4 == 0)
    return fits


def _frames(case, n, size, seed):
    """Random frames [n, h, w, 3]: uint8 over 0..255, or halves over -8..263.75 in steps of 0.25 so that both clamps of a quantiser act."""
    rng = np.random.default_rng([seed, n, size[0], size[1]])
    if case in HALF_IN:
        return (rng.integers(-32, 1056, (n, size[0], size[1], 3)) * 0.25).astype(np.float16)
    return rng.integers(0, 256, (n, size[0], size[1], 3), dtype=np.uint8)


_REF = {}


def _case(case, size):
    """(input, what the host model makes of it), computed once and left unchanged."""
    key = (case, size)
    if key not in _REF:
        x = _frames(case, N, size, seed=len(case))
        want = np.ascontiguousarray(_model(case, x))
        x.setflags(write=False)
        want.setflags(write=False)
        _REF[key] = (x, want)
    return _REF[key]


def _same(got, want):
    """Bit for bit: halves are compared as their bit patterns."""
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    if got.dtype == np.float16:
        return got.shape == want.shape and want.dtype == np.float16 and np.array_equal(got.view(np.uint16), np.ascontiguousarray(want).view(np.uint16))
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def _padded(n, frame_shape, dtype, fill):
    """A [n, stride] tensor of `fill` and its [n, *frame_shape] view: frames behind one another with a gap, the stride a multiple of 4
    bytes."""
    import torch
    isz = torch.empty((), dtype=dtype).element_size()
    elems = int(np.prod(frame_shape))
    stride = ((elems * isz + 3) // 4 * 4 + 4) // isz
    assert stride * isz % 4 == 0 and stride > elems
    big = torch.full((n, stride), fill, dtype=dtype, device=_dev())
    view = big[:, :elems].unflatten(1, tuple(frame_shape))
    assert view.stride(0) == stride and view[0].is_contiguous() and not view.is_contiguous()
    return big, view, elems


@pytest.mark.parametrize("size", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", CASES)
def test_the_shared_plan_api(case, size):
    import torch
    family = FAMILY[case]
    per = FRAMES_OUT.get(case, 1)
    x_np, want = _case(case, size)
    plan = _make(case, size)
    try:
        assert type(plan)._family == family and plan.frames_out == per and plan.device == _dev()
        x = torch.from_numpy(x_np.copy()).to(_dev())

        def vec():
            built = plan.plan()[family]
            assert built.startswith("k_") and (built.endswith("vec>") or built.endswith("general>")), built
            return built.endswith("vec>")

        def parsed():
            return dict(kv.split("=", 1) for kv in plan.last_plan().split(";") if kv)

        # plan(x) is plan.run(x); last_plan() parses to plan(); frames goes 0 -> N (source frames)
        assert vec() == _vec(case, size) and plan.plan()["frames"] == "0", plan.last_plan()
        ran = plan.run(x)
        torch.cuda.synchronize()
        assert parsed() == plan.plan() and plan.plan()["frames"] == str(N) and vec() == _vec(case, size, x, ran)
        assert tuple(ran.shape) == want.shape and ran.shape[0] == N * per and _same(ran, want)
        called = plan(x)
        torch.cuda.synchronize()
        assert called is not ran and _same(called, want)
        out = torch.empty_like(ran)
        assert plan(x, out) is out and plan.run(x, out=out) is out
        torch.cuda.synchronize()
        assert _same(out, want)

        # a batch that is a slice of a wider tensor on both sides: the frames of a packed one, and nothing written between them; the strides
        # are whole dwords, so what takes the general kernel above only for its packed 3 x 5 frames of 45 bytes takes the vec kernel here
        fill_in = 0x5A if x.dtype == torch.uint8 else 90.0
        fill_out = 0x5A if ran.dtype == torch.uint8 else 90.0
        big, view, elems = _padded(N, x.shape[1:], x.dtype, fill_in)
        big[:, :elems] = x.flatten(1)
        wide, oview, oelems = _padded(N * per, ran.shape[1:], ran.dtype, fill_out)
        assert plan.run(view, out=oview) is oview
        torch.cuda.synchronize()
        assert vec() == _vec(case, size, view, oview) == _vec(case, size) and _same(oview, want)
        assert bool((wide[:, oelems:] == fill_out).all())

        # n == 0: `out` comes back as it is and the plan string stays; through the C entry point OK and frames=0, pointers not looked at
        before = plan.last_plan()
        none = torch.empty((0,) + tuple(ran.shape[1:]), dtype=ran.dtype, device=_dev())
        assert plan.run(x[:0], out=none) is none and plan.last_plan() == before
        wide.fill_(fill_out)
        first = (None,) if family == "adeint" else ()
        run = getattr(plan.lib, f"crtfx_{family}_run")
        assert run(plan._plan, *first, view.data_ptr(), 1, oview.data_ptr(), 1, 0, None) == _lib.OK
        assert plan.plan()["frames"] == "0" and vec() == _vec(case, size)
        assert run(plan._plan, *first, None, 0, None, 0, 0, None) == _lib.OK and plan.plan()["frames"] == "0"
        assert run(plan._plan, *first, None, 0, None, 0, -1, None) == _lib.E_INVALID
        torch.cuda.synchronize()
        assert bool((wide == fill_out).all())

        # force_general: a property; the plan string follows it; the same frames, packed and sliced
        option = getattr(_lib, OPTIONS[family])
        assert option == type(plan)._force_option == 1 and plan.force_general is False
        plan.force_general = True
        assert plan.force_general is True and not vec() and plan.plan()["frames"] == "0"
        forced = plan(x)
        torch.cuda.synchronize()
        assert not vec() and plan.plan()["frames"] == str(N) and parsed() == plan.plan() and _same(forced, want)
        assert plan.run(view, out=oview) is oview
        torch.cuda.synchronize()
        assert _same(oview, want) and bool((wide[:, oelems:] == fill_out).all())
        plan.set_option(option, 0)
        assert plan.force_general is False and vec() == _vec(case, size)
        plan.set_option(option, 1)
        assert plan.force_general is True and not vec()
        with pytest.raises(_lib.CrtfxError):
            plan.set_option(option, 2)
        assert plan.force_general is True and not vec()
    finally:
        plan.close()


@pytest.mark.parametrize("case", ["canvas-u8", "canvas-half", "widen", "narrow", "deint"])
def test_a_run_across_the_group_boundary(case):
    """32769 frames of 2 x 8: the shared loop launches 32768 frames and then one, whose source and destination start 32768 strides in —
    32768 * 2 output strides under fields="both".  Frames on either side of the boundary and a dozen others against the model, on the vec
    path and on the general one."""
    import torch
    family, size, n = FAMILY[case], (2, 8), GROUP + 1
    per = FRAMES_OUT.get(case, 1)
    x_np = _frames(case, n, size, seed=11)
    picks = sorted({0, 1, GROUP - 2, GROUP - 1, GROUP} | set(np.random.default_rng(12).integers(2, GROUP - 2, 12).tolist()))
    want = np.ascontiguousarray(_model(case, x_np[picks]))
    outs = [i * per + j for i in picks for j in range(per)]
    plan = _make(case, size)
    try:
        x = torch.from_numpy(x_np).to(_dev())
        for force in (False, True):
            plan.force_general = force
            got = plan(x)
            torch.cuda.synchronize()
            built = plan.plan()
            assert built["frames"] == str(n) and built[family].endswith("general>" if force else "vec>"), built
            assert got.shape[0] == n * per and _same(got[outs], want), (case, force)
    finally:
        plan.close()
