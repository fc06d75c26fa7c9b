"""What the three resize plans take from their shared base (pythoncrt_amd/_stage.py: Handle, ResizePlan) and from the one host skeleton of
their C side (csrc/crtfx_resize_host.h), on the GPU — the counterpart of test_stage_api_gpu.py.  Four plans: IngestResize, ResizeHalf,
Resample(bicubic) on uint8 and on float16.  Calling a plan is run(), last_plan() is plan() unparsed, force_general is a property that
set_option moves, a batch that is a slice of a wider tensor gives the frames of a packed one and writes nothing between them, and the
general path's frame groups (one frame behind a fused plan, 64 otherwise) give the frames of a one-frame run.  Outputs are compared with
each other and with the exact host models (pil_resize_model, resize16_model, resample_model): equality, no tolerance."""
import numpy as np
import pytest

from pythoncrt_amd import _lib
from tests import pil_resize_model, resample_model, resize16_model

pytestmark = pytest.mark.gpu

N = 3
SHAPES = [((5, 7), (3, 4)), ((3, 5), (7, 9))]          # odd on both axes (head and tail samples exist), down and up
TALL = ((2048, 4), (1, 4))                             # no tile shape fits the LDS budget: see test_the_general_path_by_necessity
TALL_N = 65
OPTIONS = {"ingest": "INGEST_OPT_FORCE_GENERAL", "resize16": "RESIZE16_OPT_FORCE_GENERAL", "resample": "RESAMPLE_OPT_FORCE_GENERAL"}
CASES = ["ingest", "resize16", "resample-u8", "resample-half"]


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _make(case, src, dst):
    import torch
    from pythoncrt_amd import IngestResize, Resample, ResizeHalf
    if case == "ingest":
        return IngestResize(_dev(), src, dst)
    if case == "resize16":
        return ResizeHalf(_dev(), src, dst)
    return Resample(_dev(), src, dst, filter="bicubic", dtype=torch.uint8 if case == "resample-u8" else torch.float16)


def _model(case, frames, dst):
    """The host model of the plan `_make` builds, frame by frame."""
    if case == "ingest":
        return np.stack([pil_resize_model.resize(f, *dst) for f in frames])
    if case == "resize16":
        return resize16_model.resize(frames, *dst)
    if case == "resample-u8":
        return np.stack([resample_model.resize_u8(f, dst[0], dst[1], "bicubic") for f in frames])
    return resample_model.resize_half(frames, dst[0], dst[1], "bicubic")


def _frames(case, n, src, seed):
    """Random frames [n, h, w, 3]: uint8 over 0..255, or halves over -8..263.75 in steps of 0.25 so that both clamps of the quantiser act."""
    rng = np.random.default_rng([seed, n, src[0], src[1]])
    if case in ("ingest", "resample-u8"):
        return rng.integers(0, 256, (n, src[0], src[1], 3), dtype=np.uint8)
    return (rng.integers(-32, 1056, (n, src[0], src[1], 3)) * 0.25).astype(np.float16)


_REF = {}


def _case(case, n, src, dst):
    """(input, what the host model makes of it), computed once and left unchanged."""
    key = (case, n, src, dst)
    if key not in _REF:
        x = _frames(case, n, src, seed=len(case))
        want = _model(case, x if n == N else x[[0, n - 1]], dst)
        x.setflags(write=False)
        want.setflags(write=False)
        _REF[key] = (x, want)
    return _REF[key]


def _same(got, want):
    """Bit for bit: halves are compared as their bit patterns (no NaN occurs in an output, but equality is of bits all the same)."""
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    if got.dtype == np.float16:
        return got.shape == want.shape and np.array_equal(got.view(np.uint16), np.ascontiguousarray(want).view(np.uint16))
    return got.dtype == want.dtype and np.array_equal(got, want)


@pytest.mark.parametrize("src,dst", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", CASES)
def test_the_shared_plan_api(case, src, dst):
    import torch
    family = case.split("-")[0]
    x_np, want = _case(case, N, src, dst)
    plan = _make(case, src, dst)
    try:
        assert type(plan)._family == family and plan.src_size == src and plan.dst_size == dst and plan.device == _dev()
        x = torch.from_numpy(x_np.copy()).to(_dev())

        def fused():
            built = plan.plan()[family]
            assert built.startswith(f"k_{family}_fused<") or built.startswith(f"k_{family}_h+k_{family}_v"), built
            return built.startswith(f"k_{family}_fused<")

        def parsed():
            return dict(kv.split("=", 1) for kv in plan.last_plan().split(";") if kv)

        # plan(x) is plan.run(x); last_plan() parses to plan(); frames goes 0 -> N
        assert fused() and plan.plan()["frames"] == "0" and "lds" in plan.plan(), plan.last_plan()
        ran = plan.run(x)
        torch.cuda.synchronize()
        assert parsed() == plan.plan() and plan.plan()["frames"] == str(N) and fused()
        assert ran.dtype == x.dtype and tuple(ran.shape) == (N, dst[0], dst[1], 3) and _same(ran, want)
        called = plan(x)
        torch.cuda.synchronize()
        assert called is not ran and _same(called, want)
        out = torch.empty_like(ran)
        assert plan(x, out) is out and plan.run(x, out=out) is out
        torch.cuda.synchronize()
        assert _same(out, want)

        # a batch that is a slice of a wider tensor: the stride a multiple of 4 bytes and larger than a frame, on the input side ...
        isz, elems = x.element_size(), x[0].numel()
        stride = ((elems * isz + 3) // 4 * 4 + 4) // isz
        assert stride * isz % 4 == 0 and stride > elems
        fill = 0x5A if x.dtype == torch.uint8 else 90.0
        big = torch.full((N, stride), fill, dtype=x.dtype, device=_dev())
        big[:, :elems] = x.flatten(1)
        view = big[:, :elems].unflatten(1, tuple(x.shape[1:]))
        assert view.stride(0) == stride and view[0].is_contiguous() and not view.is_contiguous()
        sliced = plan(view)
        torch.cuda.synchronize()
        assert fused() and _same(sliced, want)
        oelems = ran[0].numel()                                                # ... and on the output side: nothing is written between the frames
        ostride = ((oelems * isz + 3) // 4 * 4 + 4) // isz
        assert ostride * isz % 4 == 0 and ostride > oelems
        wide = torch.full((N, ostride), fill, dtype=x.dtype, device=_dev())
        oview = wide[:, :oelems].unflatten(1, tuple(ran.shape[1:]))
        assert plan.run(view, out=oview) is oview
        torch.cuda.synchronize()
        assert fused() and _same(oview, want)
        assert bool((wide[:, oelems:] == fill).all())

        # force_general: a property; the plan string names the two general kernels; behind a fused plan the scratch holds one frame, so
        # N frames are N groups of the shared group loop; the same frames, packed and sliced
        option = getattr(_lib, OPTIONS[family])
        assert option == type(plan)._force_option == 1 and plan.force_general is False
        plan.force_general = True
        assert plan.force_general is True and not fused() and plan.plan()["frames"] == "0" and "lds" not in plan.plan()
        forced = plan(x)
        torch.cuda.synchronize()
        assert not fused() and plan.plan()["frames"] == str(N) and parsed() == plan.plan() and _same(forced, want)
        wide.fill_(fill)
        assert plan.run(view, out=oview) is oview
        torch.cuda.synchronize()
        assert _same(oview, want) and bool((wide[:, oelems:] == fill).all())
        plan.set_option(option, 0)
        assert plan.force_general is False and fused()
        plan.set_option(option, 1)
        assert plan.force_general is True and not fused()
        with pytest.raises(_lib.CrtfxError):
            plan.set_option(option, 2)
        assert plan.force_general is True and not fused()
    finally:
        plan.close()


@pytest.mark.parametrize("case", CASES)
def test_the_general_path_by_necessity(case):
    """65 frames of 2048 x 4 -> 1 x 4 (bilinear on the two BILINEAR stages, bicubic on Resample; the height 2048 passes every family's
    table checks: tests/test_stage_registry.py).  The one output row reaches all 2048 source rows and a staged source row and its
    horizontal result take at least 32 bytes of LDS, so no tile shape fits 40 960 bytes: the plan is the general one by necessity, its
    scratch holds 64 frames, and the run takes the groups 64 + 1."""
    import torch
    family = case.split("-")[0]
    src, dst = TALL
    x_np, want = _case(case, TALL_N, src, dst)
    plan = _make(case, src, dst)
    try:
        assert plan.plan()[family].startswith(f"k_{family}_h+k_{family}_v") and "lds" not in plan.plan(), plan.last_plan()
        x = torch.from_numpy(x_np.copy()).to(_dev())
        got = plan(x)
        torch.cuda.synchronize()
        assert plan.plan()[family].startswith(f"k_{family}_h+k_{family}_v") and plan.plan()["frames"] == str(TALL_N)
        got = got.cpu().numpy()
        assert got.shape == (TALL_N, 1, 4, 3) and _same(got[[0, TALL_N - 1]], want)
        single = torch.empty((1, 1, 4, 3), dtype=x.dtype, device=_dev())
        for i in range(TALL_N):                                                # every frame against a one-frame run of the same plan
            plan.run(x[i:i + 1], out=single)
            assert plan.plan()["frames"] == "1"
            assert _same(single, got[i:i + 1]), i
    finally:
        plan.close()
