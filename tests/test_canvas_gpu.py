"""The geometry stage on the GPU (include/crtfx_canvas.h, pythoncrt_amd/canvas.py) against tests/canvas_model.py: zero differing elements,
uint8 and half (compared as bits: the random halves are random bit patterns, so negatives, NaNs and infinities are among them), on both
paths, with the path taken read from plan().  Every batch lives in a larger tensor with guard elements in front of, between and behind its
frames on both sides, and the guards must come back unchanged."""
import ctypes

import numpy as np
import pytest

from pythoncrt_amd import _lib
from tests import canvas_model as model

pytestmark = pytest.mark.gpu

FILL = (7, 200, 33)             # no random frame is likely to equal it in all channels: a swapped fill or copy region shows
GUARD = {"u8": 0xA5, "f16": 0x5AA5}


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _torch_dtype(kind):
    import torch
    return torch.uint8 if kind == "u8" else torch.float16


def _np_dtype(kind):
    return np.uint8 if kind == "u8" else np.uint16


def _fill_bits(kind):
    return np.array(FILL, dtype=np.uint8) if kind == "u8" else np.array(FILL, dtype=np.float16).view(np.uint16)


def _random(kind, shape, seed):
    """Random over the whole format: every byte value; every half bit pattern."""
    rng = np.random.default_rng([seed] + list(shape))
    return rng.integers(0, 256 if kind == "u8" else 65536, shape, dtype=np.uint16).astype(_np_dtype(kind))


def _strided(kind, bits, lead, gap, tail):
    """`bits` [n, h, w, 3] placed in a flat tensor of guard elements: `lead` in front, `gap` between frames, `tail` behind.  Returns the flat
    numpy image, the flat device tensor and the [n, h, w, 3] view of it."""
    import torch
    n = bits.shape[0]
    frame = int(np.prod(bits.shape[1:]))
    flat = np.full(lead + n * (frame + gap) + tail, GUARD[kind], dtype=_np_dtype(kind))
    for i in range(n):
        flat[lead + i * (frame + gap):lead + i * (frame + gap) + frame] = bits[i].reshape(-1)
    t = torch.from_numpy(flat.view(np.uint8 if kind == "u8" else np.int16)).to(_dev())
    if kind == "f16":
        t = t.view(torch.float16)
    h, w = bits.shape[1:3]
    return flat, t, t.as_strided((n, h, w, 3), (frame + gap, w * 3, 3, 1), lead)


def _bits(kind, t):
    import torch
    return t.cpu().numpy() if kind == "u8" else t.view(torch.int16).cpu().numpy().view(np.uint16)


def _check(kind, src_size, dst_size, window, at, force_general, n=2, src_lay=(5, 3, 4), dst_lay=(8, 4, 12), seed=1, expect=None):
    """One plan, one run over n frames inside guarded tensors; the frames are the model's, the guards are untouched, the path is the one
    the header's conditions give (or `expect`)."""
    import torch
    import pythoncrt_amd as pc
    src = _random(kind, (n,) + tuple(src_size) + (3,), seed)
    s_flat, s_t, s_view = _strided(kind, src, *src_lay)
    d_flat, d_t, d_view = _strided(kind, np.full((n,) + tuple(dst_size) + (3,), GUARD[kind], dtype=_np_dtype(kind)), *dst_lay)
    plan = pc.Canvas(_dev(), src_size, dst_size, window=window, at=at, fill=FILL, dtype=_torch_dtype(kind), force_general=force_general)
    out = plan.run(s_view, out=d_view)
    torch.cuda.synchronize()
    assert out is d_view
    es = 1 if kind == "u8" else 2
    frame_bytes = dst_size[0] * dst_size[1] * 3 * es
    vec = (not force_general and frame_bytes % 4 == 0 and d_view.data_ptr() % 4 == 0 and (n <= 1 or d_view.stride(0) * es % 4 == 0))
    if expect is not None:
        assert ("vec" if vec else "general") == expect, "the case does not exercise the path it was written for"
    p = plan.plan()
    assert p == {"canvas": f"k_canvas<{kind},{'vec' if vec else 'general'}>", "frames": str(n)}, p
    fill = _fill_bits(kind)
    exp = model.canvas(src, dst_size, window=window, at=at, fill=fill)
    got_flat = _bits(kind, d_t)
    frame = dst_size[0] * dst_size[1] * 3
    lead, gap, _ = dst_lay
    want_flat = d_flat.copy()
    for i in range(n):
        want_flat[lead + i * (frame + gap):lead + i * (frame + gap) + frame] = exp[i].reshape(-1)
    bad = int((got_flat != want_flat).sum())
    assert bad == 0, (kind, src_size, dst_size, window, at, force_general, bad, np.flatnonzero(got_flat != want_flat)[:8].tolist())
    assert np.array_equal(_bits(kind, s_t), s_flat)                             # the source, guards included, is as it was
    plan.close()


# (src size, dst size, window or None, at)
SHAPES = [
    ((1, 1), (1, 1), None, (0, 0)),
    ((1, 1), (3, 3), None, (1, 1)), ((1, 1), (3, 3), None, (0, 0)), ((1, 1), (3, 3), None, (2, 2)),
    ((13, 19), (5, 7), (3, 4, 5, 7), (0, 0)),
    ((6, 8), (9, 16), None, (1, 2)),
    ((13, 19), (9, 16), (3, 4, 5, 7), (1, 2)),                                   # crop and pad in one plan
    # a window touching each source edge, and the last pixel of the frame
    ((13, 19), (5, 7), (0, 4, 5, 7), (0, 0)), ((13, 19), (5, 7), (8, 4, 5, 7), (0, 0)), ((13, 19), (5, 7), (3, 0, 5, 7), (0, 0)),
    ((13, 19), (5, 7), (3, 12, 5, 7), (0, 0)), ((13, 19), (1, 1), (12, 18, 1, 1), (0, 0)), ((13, 19), (4, 4), (12, 18, 1, 1), (3, 3)),
    ((13, 19), (8, 12), (0, 0, 1, 1), (0, 0)), ((13, 19), (8, 12), (9, 15, 4, 4), (4, 8)),
    # placements touching each destination edge
    ((6, 8), (9, 16), None, (0, 2)), ((6, 8), (9, 16), None, (3, 2)), ((6, 8), (9, 16), None, (1, 0)), ((6, 8), (9, 16), None, (1, 8)),
    ((6, 8), (9, 16), None, (3, 8)), ((6, 8), (9, 16), None, (0, 0)),
    # the whole frame as window
    ((9, 16), (9, 16), None, (0, 0)), ((7, 5), (7, 5), None, (0, 0)), ((8, 5), (8, 5), None, (0, 0)),
    # a 16-column destination: no aligned 16-byte chunk straddles a row end; a 5-column one: every chunk does
    ((6, 20), (4, 16), (1, 3, 3, 11), (1, 2)), ((6, 20), (8, 16), (0, 2, 6, 16), (1, 0)),
    ((6, 9), (8, 5), (1, 3, 5, 3), (2, 1)), ((9, 5), (12, 5), (2, 0, 7, 5), (3, 0)),
]
# win_x and dst_x so that the uint8 byte offsets 3 * win_x and 3 * dst_x are 0, 1, 2 and 3 mod 4 on each side independently
SHAPES += [((7, 24), (6, 20), (1, wx, 4, 12), (1, dx)) for wx in range(4) for dx in range(4)]
# row bytes w * 3 % 4 = 0, 1, 2, 3 on each side (w = 4, 3, 2, 1 mod 4); destination heights of 4 keep the frame a dword multiple
SHAPES += [((5, sw), (4, dw), (1, 1, 3, 4), (1, 1)) for sw in (12, 11, 10, 9) for dw in (8, 7, 6, 5)]
SHAPES += [((5, 9), (3, 7), (1, 1, 3, 4), (0, 2)), ((5, 9), (5, 5), (0, 0, 5, 5), (0, 0))]       # frame bytes no dword multiple for uint8: general


def _shape_id(s):
    return f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}-" + ("all" if s[2] is None else "w" + "_".join(map(str, s[2]))) + f"-at{s[3][0]}_{s[3][1]}"


@pytest.mark.parametrize("force_general", [False, True], ids=["auto", "general"])
@pytest.mark.parametrize("kind", ["u8", "f16"])
@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_shapes(shape, kind, force_general):
    src_size, dst_size, window, at = shape
    _check(kind, src_size, dst_size, window, at, force_general)


@pytest.mark.parametrize("kind", ["u8", "f16"])
def test_source_base_at_every_byte_offset_stays_on_vec(kind):
    """Nothing is asked of the source: a frame that starts 1, 2 or 3 elements into its tensor (for uint8: off a dword) and whose gap makes
    every frame start elsewhere still runs on vec, and its first and last dwords — which stick out of the frame — are read byte-wise."""
    for lead in (0, 1, 2, 3):
        for gap in (0, 1, 2, 7):
            _check(kind, (7, 5), (8, 6), None, (1, 1), False, n=3, src_lay=(lead, gap, 2), expect="vec")
            _check(kind, (6, 8), (6, 8), None, (0, 0), False, n=3, src_lay=(lead, gap, 0), expect="vec")      # identity: the window is the frame
            _check(kind, (9, 5), (3, 4), (6, 1, 3, 4), (0, 0), False, n=3, src_lay=(lead, gap, 0), expect="vec")   # the window ends with the frame


@pytest.mark.parametrize("kind", ["u8", "f16"])
def test_batches_with_unequal_strides_and_bases_that_leave_vec(kind):
    shape = ((13, 19), (8, 16), (3, 4, 5, 7), (1, 2))
    _check(kind, *shape, False, n=3, src_lay=(5, 9, 4), dst_lay=(8, 20, 12), expect="vec")
    _check(kind, *shape, True, n=3, src_lay=(5, 9, 4), dst_lay=(8, 20, 12), expect="general")
    _check(kind, *shape, False, n=1, dst_lay=(16, 3, 5), expect="vec")                          # one frame: the stride does not count
    _check(kind, *shape, False, n=3, dst_lay=(16, 16, 0), expect="vec")                         # 16-byte aligned base and stride: 16-byte stores
    if kind == "u8":
        for lead in (1, 2, 3):
            _check(kind, *shape, False, n=3, dst_lay=(lead, 4, 7), expect="general")            # the base is off a dword
        for gap in (1, 2, 3):
            _check(kind, *shape, False, n=3, dst_lay=(8, gap, 7), expect="general")             # the stride is
    else:
        _check(kind, *shape, False, n=3, dst_lay=(1, 4, 7), expect="general")                   # an odd element: 2 mod 4 bytes
        _check(kind, *shape, False, n=3, dst_lay=(8, 1, 7), expect="general")


@pytest.mark.parametrize("kind", ["u8", "f16"])
def test_no_frames_and_the_refusals_of_run(kind):
    import torch
    import pythoncrt_amd as pc
    dt = _torch_dtype(kind)
    plan = pc.Canvas(_dev(), (6, 8), (9, 16), at=(1, 2), fill=FILL, dtype=dt)
    assert plan.plan() == {"canvas": f"k_canvas<{kind},vec>", "frames": "0"}
    out = plan.run(torch.empty((0, 6, 8, 3), dtype=dt, device=_dev()))
    assert tuple(out.shape) == (0, 9, 16, 3) and out.dtype == dt
    plan.force_general = True
    assert plan.force_general and plan.plan()["canvas"] == f"k_canvas<{kind},general>"
    plan.force_general = False
    src = torch.zeros((2, 6, 8, 3), dtype=dt, device=_dev())
    with pytest.raises(_lib.CrtfxError):
        plan.run(src.to(torch.float32))
    with pytest.raises(ValueError, match="frames must be"):
        plan.run(src[:, :5])
    with pytest.raises(ValueError, match="out must be"):
        plan.run(src, out=torch.empty((2, 9, 15, 3), dtype=dt, device=_dev()))
    with pytest.raises(ValueError, match="contiguous"):
        plan.run(torch.zeros((2, 6, 16, 3), dtype=dt, device=_dev())[:, :, ::2])
    # through the C-ABI: a stride shorter than a frame, n < 0, a null pointer, overlapping frames, and for half frames an odd base or stride;
    # all are refused before anything is launched
    lib, es = plan.lib, src.element_size()
    dst = torch.empty((2, 9, 16, 3), dtype=dt, device=_dev())
    sb, db = 6 * 8 * 3 * es, 9 * 16 * 3 * es
    st = torch.cuda.current_stream().cuda_stream
    run = lambda *a: lib.crtfx_canvas_run(plan._plan, *a, st)      # noqa: E731
    assert run(src.data_ptr(), sb, dst.data_ptr(), db, 2) == _lib.OK
    assert run(src.data_ptr(), sb - 4, dst.data_ptr(), db, 2) == _lib.E_INVALID and "smaller than a frame" in plan._fn("last_error")(plan._plan).decode()
    assert run(src.data_ptr(), sb, dst.data_ptr(), db - 4, 2) == _lib.E_INVALID
    assert run(src.data_ptr(), sb, dst.data_ptr(), db, -1) == _lib.E_INVALID
    assert run(None, sb, dst.data_ptr(), db, 1) == _lib.E_INVALID and run(src.data_ptr(), sb, None, db, 1) == _lib.E_INVALID
    assert run(dst.data_ptr(), sb, dst.data_ptr() + 4 * es, db, 1) == _lib.E_INVALID and "overlap" in plan._fn("last_error")(plan._plan).decode()
    if kind == "f16":
        for a in ((src.data_ptr() + 1, sb, dst.data_ptr(), db, 1), (src.data_ptr(), sb, dst.data_ptr() + 1, db, 1),
                  (src.data_ptr(), sb + 1, dst.data_ptr(), db, 2), (src.data_ptr(), sb, dst.data_ptr(), db + 1, 2)):
            assert run(*a) == _lib.E_INVALID and "even" in plan._fn("last_error")(plan._plan).decode(), a
    assert lib.crtfx_canvas_set_option(plan._plan, 9, 1) == _lib.E_INVALID and lib.crtfx_canvas_set_option(plan._plan, 1, 2) == _lib.E_INVALID
    torch.cuda.synchronize()
    plan.close()


@pytest.mark.parametrize("kind", ["u8", "f16"])
def test_full_size_pillarbox_with_a_misaligned_window(kind):
    """1080 x 1440 placed at dx = 241 on 1080 x 1920, two frames, both paths over the same frames."""
    import torch
    import pythoncrt_amd as pc
    src = _random(kind, (2, 1080, 1440, 3), 5)
    exp = model.canvas(src, (1080, 1920), at=(0, 241), fill=_fill_bits(kind))
    t = torch.from_numpy(src.view(np.uint8 if kind == "u8" else np.int16)).to(_dev())
    t = t if kind == "u8" else t.view(torch.float16)
    for force in (False, True):
        plan = pc.Canvas(_dev(), (1080, 1440), (1080, 1920), at=(0, 241), fill=FILL, dtype=_torch_dtype(kind), force_general=force)
        got = _bits(kind, plan.run(t))
        assert plan.plan() == {"canvas": f"k_canvas<{kind},{'general' if force else 'vec'}>", "frames": "2"}
        assert int((got != exp).sum()) == 0, (kind, force, int((got != exp).sum()))
        plan.close()
