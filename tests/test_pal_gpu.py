"""The PAL composite-video stage on the GPU (include/crtfx_pal.h) against tests/pal_model.py: both sample types, both signals, both decoder
chroma filters, both decoders, phase errors, crawl on and off, both paths.  Every comparison is exact: no element may differ."""
import itertools

import numpy as np
import pytest

from pythoncrt_amd import _lib
from pythoncrt_amd import pal as pal_mod
from tests import pal_model as model

pytestmark = pytest.mark.gpu

GUARD = 0xA5
SEG = 488                               # the pixels of a row one wave of the vec kernels takes (include/crtfx_pal.h)
R = pal_mod.STRIP                       # ... and the rows of its strip
# heights around the strip — one row (its own partner), two, three, a strip less a row, a strip, a strip and a row (the second strip's first
# fill is the last row of the first), two strips and a row — at a width narrower than every halo and one wider; widths narrower than the
# halo, one segment -8 / +0 / +8, two segments + 24, at three rows: the row-0 rule and both V switches
SHAPES = [(h, w) for h in (1, 2, 3, R - 1, R, R + 1, 2 * R + 1) for w in (8, 40)] + [(3, w) for w in (1, 3, 5, 16, SEG - 8, SEG, SEG + 8, 2 * SEG + 24)]
RUNS = ((1, 0, True), (2, 1, True), (3, 2, False), (5, 3, True), (5, 0, False), (3, 2, True))     # (n, index, crawl): every index mod 4 with crawl
DTYPES = {"u8": np.uint8, "f16": np.float16}
COMBOS = list(itertools.product(model.SIGNALS, model.CHROMAS, model.DECODERS))
PHASES = (0, 20, -90, 180)
STRIP_CASES = [(1, 8), (R - 1, 40), (R, 8), (R + 1, 40), (2 * R + 1, 16), (3, SEG + 8)]             # one shape per strip case


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _torch_dtype(pix):
    import torch
    return torch.uint8 if pix == "u8" else torch.float16


def _plan(size, pix, signal="composite", chroma="sharp", decoder="delay", crawl=True, phase=0, force=False):
    import pythoncrt_amd as pc
    return pc.PalSignal(_dev(), size, signal=signal, chroma=chroma, crawl=crawl, decoder=decoder, phase=phase, dtype=_torch_dtype(pix), force_general=force)


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
    return n <= 1 or not ((src.stride(0) * src.element_size()) | (dst.stride(0) * dst.element_size())) & 3


def _name(signal, chroma, decoder, pix, vec):
    return f"k_pal<{signal},{chroma},{decoder},{pix},{'vec' if vec else 'general'}>"


def test_the_strip_height_is_one_of_the_candidates():
    import os
    hdr = " ".join(open(os.path.join(_lib.ROOT, "include", "crtfx_pal.h")).read().replace(" * ", " ").split())
    assert R in (8, 16, 32) and f"a strip of {R} consecutive rows" in hdr


@pytest.mark.parametrize("force", [False, True], ids=["auto", "forced"])
@pytest.mark.parametrize("pix", list(DTYPES))
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_counts_indices_and_crawl_against_the_model(size, pix, force):
    import torch
    src = _source(pix, (5,) + size + (3,), [size[0], size[1]])
    x = torch.from_numpy(src).to(_dev())
    for signal, chroma, decoder in COMBOS:
        plans = {crawl: _plan(size, pix, signal, chroma, decoder, crawl, 0, force) for crawl in (True, False)}
        for n, index, crawl in RUNS:
            plan = plans[crawl]
            out = plan.run(x[:n], index=index)
            torch.cuda.synchronize()
            assert tuple(out.shape) == (n,) + size + (3,)
            exp = model.pal(src[:n], signal, chroma, crawl, index, decoder, 0)
            assert _same(out.cpu().numpy(), exp) == 0, (size, pix, signal, chroma, decoder, force, n, index, crawl)
            vec = _vec_expected(size[1], x[:n], out, n, force)
            assert plan.plan() == {"pal": _name(signal, chroma, decoder, pix, vec), "frames": str(n)}, plan.last_plan()
            if not force:                                                      # fresh allocations are aligned: the vec path wherever the width lets it
                assert vec == (size[1] % 8 == 0)
        for plan in plans.values():
            plan.close()


@pytest.mark.parametrize("force", [False, True], ids=["auto", "forced"])
@pytest.mark.parametrize("pix", list(DTYPES))
@pytest.mark.parametrize("phase", PHASES)
def test_phase_errors_against_the_model(phase, pix, force):
    """One shape per strip case, every signal, filter and decoder, at index 1 with crawl."""
    import torch
    for size in STRIP_CASES:
        src = _source(pix, (2,) + size + (3,), [size[0], size[1], phase + 180])
        x = torch.from_numpy(src).to(_dev())
        for signal, chroma, decoder in COMBOS:
            plan = _plan(size, pix, signal, chroma, decoder, True, phase, force)
            got = plan.run(x, index=1).cpu().numpy()
            assert _same(got, model.pal(src, signal, chroma, True, 1, decoder, phase)) == 0, (size, signal, chroma, decoder, phase)
            plan.close()


@pytest.mark.parametrize("force", [False, True], ids=["vec", "general"])
def test_every_half_pattern(force):
    """All 65 536 half patterns in each row of two 2 x 21848 frames, rolled differently: every pattern is quantised as a centre and as a
    neighbour of every tap, in a row and in its partner."""
    import torch
    w = 21848                                                                   # 8 * 2731 pixels: 65 544 samples per row, 45 segments
    pats = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    src = np.stack([np.stack([np.concatenate([np.roll(pats, 7919 * (2 * f + y)), pats[:8]]) for y in range(2)]) for f in range(2)])
    src = src.view(np.float16).reshape(2, 2, w, 3)
    x = torch.from_numpy(src).to(_dev())
    for signal, chroma, decoder in (("composite", "sharp", "delay"), ("composite", "soft", "simple"), ("svideo", "sharp", "simple"), ("svideo", "soft", "delay")):
        plan = _plan((2, w), "f16", signal, chroma, decoder, True, 20, force)
        got = plan.run(x, index=1).cpu().numpy()
        assert plan.plan() == {"pal": _name(signal, chroma, decoder, "f16", not force), "frames": "2"}
        assert _same(got, model.pal(src, signal, chroma, True, 1, decoder, 20)) == 0, (signal, chroma, decoder)
        plan.close()


@pytest.mark.parametrize("force", [False, True], ids=["vec", "general"])
@pytest.mark.parametrize("pix", list(DTYPES))
def test_the_clamps_on_extreme_noise(pix, force):
    """{0, M} noise drives the results below 0 and above M (tests/test_pal_tables.py shows that it does)."""
    import torch
    size = (R + 1, 2 * SEG + 24)
    src = (np.random.default_rng(5).integers(0, 2, (2,) + size + (3,)) * 255).astype(DTYPES[pix])
    x = torch.from_numpy(src).to(_dev())
    for signal, chroma, decoder in COMBOS:
        v = model.cascade(model.codes(src), signal, chroma, True, 0, decoder, 45)
        assert (v < 0).any() and (v > model.top(DTYPES[pix])).any()
        plan = _plan(size, pix, signal, chroma, decoder, True, 45, force)
        assert _same(plan.run(x).cpu().numpy(), model.pal(src, signal, chroma, True, 0, decoder, 45)) == 0, (signal, chroma, decoder)
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


@pytest.mark.parametrize("signal,chroma,decoder", [("composite", "soft", "delay"), ("svideo", "sharp", "simple")])
@pytest.mark.parametrize("pix", list(DTYPES))
@pytest.mark.parametrize("size", [(3, 8), (R + 1, 24), (5, 13)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_base_offset_inside_guards(size, pix, signal, chroma, decoder):
    """uint8 frames at byte offsets 0..3, half frames at 0 and 2, three frames, source and destination strides that differ and are a few
    bytes longer than a frame: the bytes are the model's, the path is the one the header's conditions give, and no byte outside the
    frames changes, in the source or in the destination."""
    import torch
    h, w = size
    dt, item = _torch_dtype(pix), (1 if pix == "u8" else 2)
    fb = h * w * 3 * item
    offsets = range(4) if pix == "u8" else (0, 2)
    seen = set()
    n = 3
    plan = _plan(size, pix, signal, chroma, decoder, True, 20)
    for s_off, d_off in itertools.product(offsets, offsets):
        for s_gap, d_gap in ((0, 4), (8, 0), (2, 6), (4, 8)) if pix == "f16" else ((0, 4), (8, 0), (3, 1), (1, 4)):
            src_np = _source(pix, (n,) + size + (3,), [h, w, s_off, d_off, s_gap])
            sb, s = _guarded(n, fb, fb + s_gap, s_off, dt)
            db, d = _guarded(n, fb, fb + d_gap, d_off, dt)
            s.copy_(torch.from_numpy(src_np.reshape(n, -1)).to(_dev()))
            s4 = s.as_strided((n, h, w, 3), (s.stride(0), w * 3, 3, 1))
            d4 = d.as_strided((n, h, w, 3), (d.stride(0), w * 3, 3, 1))
            plan.run(s4, out=d4, index=1)
            torch.cuda.synchronize()
            vec = _vec_expected(w, s4, d4, n)
            seen.add(vec)
            assert plan.plan()["pal"] == _name(signal, chroma, decoder, pix, vec), (s_off, d_off, s_gap, d_gap, plan.last_plan())
            assert _same(d4.cpu().numpy(), model.pal(src_np, signal, chroma, True, 1, decoder, 20)) == 0, (s_off, d_off, s_gap, d_gap)
            assert _guards_intact(db, n, fb, fb + d_gap, d_off) and _guards_intact(sb, n, fb, fb + s_gap, s_off)
            assert _same(s4.cpu().numpy(), src_np) == 0
    plan.close()
    assert seen == ({False} if w % 8 else {True, False})


@pytest.mark.parametrize("signal,chroma,decoder", COMBOS)
@pytest.mark.parametrize("pix", list(DTYPES))
def test_no_frames_a_long_batch_and_the_call_forms(pix, signal, chroma, decoder):
    import torch
    size = (3, 8)
    plan = _plan(size, pix, signal, chroma, decoder)
    src_np = _source(pix, (65,) + size + (3,), 65)
    x = torch.from_numpy(src_np).to(_dev())
    out = plan.run(x)                                                          # 65 frames of 3 x 8 in one grid
    torch.cuda.synchronize()
    assert plan.plan() == {"pal": _name(signal, chroma, decoder, pix, True), "frames": "65"} and out.shape[0] == 65
    assert _same(out.cpu().numpy(), model.pal(src_np, signal, chroma, True, 0, decoder)) == 0
    assert torch.equal(plan(x).view(torch.uint8), plan.run(x).view(torch.uint8))       # plan(x) == plan.run(x)
    empty = plan.run(x[:0])
    assert tuple(empty.shape) == (0,) + size + (3,) and empty.dtype == out.dtype
    keep = out.clone()
    assert plan.run(x[:0], out=out[:0]).data_ptr() == out[:0].data_ptr()       # n = 0: `out` comes back untouched
    # n = 0 through the C entry point: nothing runs, nothing is written, nothing is asked of the pointers
    st = torch.cuda.current_stream().cuda_stream
    assert plan.lib.crtfx_pal_run(plan._plan, 0, x.data_ptr(), 0, out.data_ptr(), 0, 0, st) == _lib.OK
    assert plan.lib.crtfx_pal_run(plan._plan, 5, None, 0, None, 0, 0, st) == _lib.OK
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.uint8), keep.view(torch.uint8)) and plan.plan()["frames"] == "0"
    # force_general switches the plan string and not the bytes
    plan.force_general = True
    assert plan.force_general and plan.plan()["pal"] == _name(signal, chroma, decoder, pix, False)
    forced = plan.run(x)
    torch.cuda.synchronize()
    assert plan.plan() == {"pal": _name(signal, chroma, decoder, pix, False), "frames": "65"} and torch.equal(forced.view(torch.uint8), out.view(torch.uint8))
    plan.force_general = False
    assert plan.plan()["pal"] == _name(signal, chroma, decoder, pix, True)
    plan.close()


@pytest.mark.parametrize("force", [False, True], ids=["vec", "general"])
@pytest.mark.parametrize("index", [0, 3])
def test_one_batch_across_the_launch_group_boundary(index, force):
    """The launch is grouped by grid.z, 32768 frames per launch: 32769 frames of 2 x 8 need a second launch, whose one frame continues the
    count of the first (2 x 1 has no vec path; it runs forced as the general kernel of 2 x 8 does)."""
    import torch
    n = 32768 + 1
    for size in ((2, 1),) if force else ((2, 8),):
        src = np.random.default_rng(n + index).integers(0, 256, (n,) + size + (3,), dtype=np.uint8)
        plan = _plan(size, "u8", "composite", "sharp", "delay", True, 20, force)
        out = plan.run(torch.from_numpy(src).to(_dev()), index=index)
        torch.cuda.synchronize()
        assert out.shape[0] == n and plan.plan() == {"pal": _name("composite", "sharp", "delay", "u8", not force), "frames": str(n)}
        assert _same(out.cpu().numpy(), model.pal(src, "composite", "sharp", True, index, "delay", 20)) == 0
        plan.close()


@pytest.mark.parametrize("pix", list(DTYPES))
def test_push_counts_frames_across_batches(pix):
    """push in batches of 1 + 4 + 2 is one run of 7 — the counter crosses 4 inside the second batch; reset() sets the count."""
    import torch
    size = (3, 16)
    src = _source(pix, (7,) + size + (3,), 7)
    x = torch.from_numpy(src).to(_dev())
    plan = _plan(size, pix, "composite", "soft", "delay", True, 20)
    whole = model.pal(src, "composite", "soft", True, 0, "delay", 20)
    assert _same(plan.run(x).cpu().numpy(), whole) == 0
    got = torch.cat([plan.push(x[:1]), plan.push(x[1:5]), plan.push(x[5:])])
    assert _same(got.cpu().numpy(), whole) == 0 and plan._index == 7
    assert _same(plan.push(x[:2]).cpu().numpy(), model.pal(src[:2], "composite", "soft", True, 7, "delay", 20)) == 0 and plan._index == 9
    plan.push(x[:0])
    assert plan._index == 9
    plan.reset()
    assert _same(plan.push(x[:3]).cpu().numpy(), whole[:3]) == 0
    plan.reset(4)
    out = torch.empty_like(x[:3])
    assert plan.push(x[4:], out=out).data_ptr() == out.data_ptr() and _same(out.cpu().numpy(), whole[4:]) == 0
    assert _same(plan.run(x[1:2], index=1).cpu().numpy(), whole[1:2]) == 0 and plan._index == 7      # run() is stateless
    assert _same(plan.run(x[1:2], index=5).cpu().numpy(), whole[1:2]) == 0                          # t and t + 4
    for other in (0, 2, 3):
        assert _same(whole[1:2], model.pal(src[1:2], "composite", "soft", True, other, "delay", 20)) != 0    # and the index matters
    plan.close()


@pytest.mark.parametrize("pix", list(DTYPES))
def test_run_refusals(pix):
    """The refusals of crtfx_signal_run: a negative first index, odd half bases and strides, overlapping ranges, short strides, null
    pointers, n < 0 and wrong tensors are refused, and no refused call writes anything."""
    import torch
    from pythoncrt_amd._lib import CrtfxError
    size, n = (3, 8), 4
    plan = _plan(size, pix)
    fb = 72 * (1 if pix == "u8" else 2)
    src = torch.zeros(n * fb + 16, dtype=torch.uint8, device=_dev())
    dst = torch.full((n * fb + 16,), 7, dtype=torch.uint8, device=_dev())
    run, err = plan.lib.crtfx_pal_run, plan.lib.crtfx_pal_last_error
    st = torch.cuda.current_stream().cuda_stream
    sp, dp = src.data_ptr(), dst.data_ptr()
    for bad in (-1, -2 ** 40):
        assert run(plan._plan, bad, sp, fb, dp, fb, 1, st) == _lib.E_INVALID and b"first_index" in err(plan._plan)
        assert run(plan._plan, bad, sp, fb, dp, fb, 0, st) == _lib.E_INVALID
    if pix == "f16":
        assert run(plan._plan, 0, sp + 1, fb, dp, fb, 1, st) == _lib.E_INVALID and b"even" in err(plan._plan)
        assert run(plan._plan, 0, sp, fb, dp + 1, fb, 1, st) == _lib.E_INVALID and b"even" in err(plan._plan)
        assert run(plan._plan, 0, sp, fb + 1, dp, fb, 2, st) == _lib.E_INVALID and b"even" in err(plan._plan)
        assert run(plan._plan, 0, sp, fb, dp, fb + 1, 2, st) == _lib.E_INVALID and b"even" in err(plan._plan)
    assert run(plan._plan, 0, sp, fb - 2, dp, fb, 2, st) == _lib.E_INVALID and b"strides" in err(plan._plan)
    assert run(plan._plan, 0, sp, fb, dp, fb - 2, 2, st) == _lib.E_INVALID and b"strides" in err(plan._plan)
    assert run(plan._plan, 0, None, fb, dp, fb, 1, st) == _lib.E_INVALID and b"null" in err(plan._plan)
    assert run(plan._plan, 0, sp, fb, None, fb, 1, st) == _lib.E_INVALID
    assert run(plan._plan, 0, sp, fb, dp, fb, -1, st) == _lib.E_INVALID and b"n = -1" in err(plan._plan)
    both = torch.zeros(n * 2 * fb + 8, dtype=torch.uint8, device=_dev())
    bp = both.data_ptr()
    for s_at, d_at in ((0, 0), (0, n * fb - 2), (2 * fb - 2, 0), (0, fb)):
        assert run(plan._plan, 0, bp + s_at, fb, bp + d_at, fb, n, st) == _lib.E_INVALID and b"overlap" in err(plan._plan), (s_at, d_at)
    assert run(plan._plan, 2 ** 40 + 1, bp, fb, bp + n * fb, fb, n, st) == _lib.OK       # touching ranges do not overlap; a large index is its value mod 4
    torch.cuda.synchronize()
    assert int((dst != 7).sum()) == 0 and int(src.sum()) == 0
    x = torch.zeros((n,) + size + (3,), dtype=_torch_dtype(pix), device=_dev())
    for bad in (-1, 1.0, None, True):
        with pytest.raises(ValueError, match="index"):
            plan.run(x, index=bad)
    with pytest.raises(CrtfxError) as e:
        plan.run(x.to(torch.float32))
    assert e.value.code == _lib.E_UNSUPPORTED
    with pytest.raises(ValueError, match="frames must be"):
        plan.run(x[:, :2])
    for bad in (n - 1, n + 1):
        with pytest.raises(ValueError, match="out must be"):
            plan.run(x, out=torch.empty((bad,) + size + (3,), dtype=x.dtype, device=_dev()))
    with pytest.raises(CrtfxError) as e:
        plan.set_option(99, 1)
    assert e.value.code == _lib.E_INVALID and "option" in str(e.value)
    with pytest.raises(CrtfxError) as e:
        _plan((0, 8), pix)
    assert e.value.code == _lib.E_INVALID and "h = 0" in str(e.value)
    plan.close()


@pytest.mark.parametrize("size", [(576, 720), (1080, 1920)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pix", list(DTYPES))
def test_a_full_size_batch(size, pix):
    import torch
    n = 8
    signal, chroma, decoder = ("composite", "sharp", "delay") if pix == "u8" else ("composite", "soft", "delay")
    src_np = model.noise(size[0], size[1], n=n, dtype=DTYPES[pix], seed=size[0])
    plan = _plan(size, pix, signal, chroma, decoder, True, 20)
    out = plan.run(torch.from_numpy(src_np).to(_dev()), index=1)
    torch.cuda.synchronize()
    assert plan.plan() == {"pal": _name(signal, chroma, decoder, pix, True), "frames": str(n)}
    assert _same(out.cpu().numpy(), model.pal(src_np, signal, chroma, True, 1, decoder, 20)) == 0
    plan.close()
