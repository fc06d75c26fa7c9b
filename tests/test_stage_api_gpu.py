"""What the ten format-stage plans take from their shared base (pythoncrt_amd/_stage.py), on the GPU: calling a plan is run(), last_plan()
is plan() unparsed, force_general is a property that set_option moves, and a batch that is a slice of a larger tensor (the batch stride
passed in bytes) gives the frames of a packed one.  Every class, every layout, 2-frame batches of 2 x 8 (vec) and 3 x 5 (general; odd on
both axes).  What the kernels compute is held elsewhere (test_unpack_gpu.py ... test_deep444_gpu.py): here outputs are compared with each
other only."""
import numpy as np
import pytest

from pythoncrt_amd import _lib, formats

pytestmark = pytest.mark.gpu

N = 2
SIZES = [(2, 8), (3, 5)]
OPTIONS = {"unpack": "UNPACK_OPT_FORCE_GENERAL", "egress": "EGRESS_OPT_FORCE_GENERAL", "unpack10": "UNPACK10_OPT_FORCE_GENERAL",
           "egress10": "EGRESS10_OPT_FORCE_GENERAL", "unpack422": "UNPACK422_OPT_FORCE_GENERAL", "egress422": "EGRESS422_OPT_FORCE_GENERAL",
           "unpack444": "UNPACK444_OPT_FORCE_GENERAL", "egress444": "EGRESS444_OPT_FORCE_GENERAL"}
CASES = [(kind, fmt) for fmt in formats.FORMATS for kind in ("source", "egress")]


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _input(cls, kind, size, fmt, seed):
    """A flat [N, elements] batch of what the plan reads, and the shape of one frame: random bytes for a source plan, random RGB for an
    egress plan (uint8 over 0..255, or halves over -8..263.75 in steps of 0.25 so that both clamps act)."""
    import torch
    h, w = size
    rng = np.random.default_rng(seed)
    if kind == "source":
        fb = formats.frame_bytes(h, w, fmt)
        return torch.from_numpy(rng.integers(0, 256, (N, fb), dtype=np.uint8)), (fb,)
    if cls._rgb == "uint8":
        return torch.from_numpy(rng.integers(0, 256, (N, h * w * 3), dtype=np.uint8)), (h, w, 3)
    return torch.from_numpy((rng.integers(-32, 1056, (N, h * w * 3)) * 0.25).astype(np.float16)), (h, w, 3)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind,fmt", CASES, ids=[f"{k}-{f}" for k, f in CASES])
def test_the_shared_plan_api(kind, fmt, size):
    import torch
    family = formats.FORMATS[fmt]
    cls = family.source if kind == "source" else family.egress
    vec = size == (2, 8)
    h, w = size
    plan = cls(_dev(), size, layout=fmt)
    try:
        assert plan.size == size and plan.layout == fmt and plan.frame_bytes == formats.frame_bytes(h, w, fmt) and plan.device == _dev()
        flat, frame = _input(cls, kind, size, fmt, seed=h * 100 + w)
        x = flat.to(_dev()).unflatten(1, frame) if len(frame) > 1 else flat.to(_dev())

        def path():
            built = plan.plan()[cls._family]
            assert built.endswith(",vec>") or built.endswith(",general>"), built
            return built.rsplit(",", 1)[1][:-1]

        def parsed():
            return dict(kv.split("=", 1) for kv in plan.last_plan().split(";") if kv)

        # plan(x) is plan.run(x); last_plan() parses to plan()
        assert path() == ("vec" if vec else "general") and plan.plan()["frames"] == "0"
        ran = plan.run(x)
        torch.cuda.synchronize()
        assert parsed() == plan.plan() == {cls._family: plan.plan()[cls._family], "frames": str(N)} and path() == ("vec" if vec else "general")
        called = plan(x)
        torch.cuda.synchronize()
        want = ran.cpu().numpy()
        assert called is not ran and np.array_equal(called.cpu().numpy(), want)
        assert want.shape == ((N, h, w, 3) if kind == "source" else (N, plan.frame_bytes))
        assert want.dtype == (np.dtype(cls._rgb) if kind == "source" else np.uint8)
        out = torch.empty_like(ran)
        assert plan(x, out) is out and plan.run(x, out=out) is out
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want)

        # a batch that is a slice of a larger tensor: the stride a multiple of 4 bytes (so that the vec path stays open) and larger than a frame
        isz, elems = flat.element_size(), flat.shape[1]
        stride = ((elems * isz + 3) // 4 * 4 + 4) // isz
        assert stride * isz % 4 == 0 and stride > elems
        big = torch.full((N, stride), 0x5A if flat.dtype == torch.uint8 else 90.0, dtype=flat.dtype, device=_dev())
        big[:, :elems] = flat.to(_dev())
        view = big[:, :elems].unflatten(1, frame) if len(frame) > 1 else big[:, :elems]
        assert view.stride(0) == stride and view[0].is_contiguous() and not view.is_contiguous()
        sliced = plan(view)
        torch.cuda.synchronize()
        assert path() == ("vec" if vec else "general"), plan.last_plan()
        assert np.array_equal(sliced.cpu().numpy(), want)
        osz, oelems = ran.element_size(), ran[0].numel()                                                     # ... and on the output side
        ostride = ((oelems * osz + 3) // 4 * 4 + 4) // osz
        wide = torch.zeros((N, ostride), dtype=ran.dtype, device=_dev())
        oview = wide[:, :oelems].unflatten(1, tuple(ran.shape[1:])) if ran.dim() > 2 else wide[:, :oelems]
        assert plan.run(view, out=oview) is oview
        torch.cuda.synchronize()
        assert path() == ("vec" if vec else "general") and np.array_equal(oview.cpu().numpy(), want)
        assert bool((wide[:, oelems:] == 0).all())                              # nothing written between the frames

        # force_general: a property; set_option with the family's number moves it; the general build gives the same frames
        option = getattr(_lib, OPTIONS[cls._family])
        assert option == cls._force_option and plan.force_general is False
        plan.force_general = True
        assert plan.force_general is True and path() == "general" and plan.plan()["frames"] == "0"
        forced = plan(x)
        torch.cuda.synchronize()
        assert path() == "general" and plan.plan()["frames"] == str(N) and np.array_equal(forced.cpu().numpy(), want)
        plan.set_option(option, 0)
        assert plan.force_general is False and path() == ("vec" if vec else "general")
        plan.set_option(option, 1)
        assert plan.force_general is True and path() == "general"
        with pytest.raises(_lib.CrtfxError):
            plan.set_option(option, 2)
        assert plan.force_general is True
    finally:
        plan.close()
