"""The 10-bit 4:4:4 pair on the GPU: UnpackDeep444 (k_unpack10_444) and EgressDeep444 (k_egress10_444), vec and general path, planar and
x2rgb10le, against the integer host model of tests/deep444_model.py — equality means zero differing bits, halves compared as their uint16
patterns — and process_frames / the CLI with the new formats on both ends and mixed with p010le against the models around a half
FramePipeline."""
import dataclasses

import numpy as np
import pytest

from pythoncrt_amd import _lib
from tests import deep444_model as model
from tests import deep_model

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (2, 3), (3, 5), (1, 8), (16, 64), (34, 136), (37, 131), (270, 480)]
FORMATS = list(model.FORMATS)
TOKEN = {"yuv444p10le": "planar", "gbrp10le": "planar", "x2rgb10le": "x2rgb10le"}


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _name(kind, fmt, vec):
    return f"k_{kind}10_444<{TOKEN[fmt]},{'vec' if vec else 'general'}>"


def _bits(a):
    """The uint16 patterns of a float16 array / the uint16 words of a packed uint8 one."""
    return np.ascontiguousarray(a).view(np.uint16)


_CACHE = {}


def _frames(size, fmt, seed=0):
    """The three packed test frames of a size in the layout of `fmt`, uint8 [3, frame_bytes] (the same samples P0, P1, P2 in every format),
    and the model's halves of them under `fmt`'s table at bt601 / tv (computed once per size, seed and format)."""
    key = (size, seed)
    if key not in _CACHE:
        _CACHE[key] = {"planar": model.images(*size, seed=seed)}
    c = _CACHE[key]
    if fmt not in c:
        packed = np.stack([model.relayout(p, size[0], size[1], fmt) for p in c["planar"]])
        c[fmt] = (packed, np.stack([model.unpack(p, size[0], size[1], fmt) for p in packed]))
    return c[fmt]


def _unpack(packed_np, size, fmt, force_general=False, matrix="bt601", rng="tv"):
    """(float16[n, h, w, 3] from the device, the plan's words) for a stack of packed frames."""
    import torch
    from pythoncrt_amd import UnpackDeep444
    plan = UnpackDeep444(_dev(), size, layout=fmt, matrix=matrix, range=rng)
    if force_general:
        plan.set_option(_lib.UNPACK444_OPT_FORCE_GENERAL, 1)
    out = plan.run(torch.from_numpy(packed_np).to(_dev()))
    torch.cuda.synchronize()
    got, how = out.cpu().numpy(), plan.plan()
    assert got.dtype == np.float16 and got.shape == (packed_np.shape[0],) + tuple(size) + (3,)
    plan.close()
    return got, how


def _egress(frames_np, fmt, force_general=False, matrix="bt601", rng="tv"):
    """(uint8[n, frame_bytes] from the device, the plan's words) for a stack of float16 frames."""
    import torch
    from pythoncrt_amd import EgressDeep444
    size = tuple(frames_np.shape[1:3])
    plan = EgressDeep444(_dev(), size, layout=fmt, matrix=matrix, range=rng)
    if force_general:
        plan.set_option(_lib.EGRESS444_OPT_FORCE_GENERAL, 1)
    out = plan.run(torch.from_numpy(frames_np).to(_dev()))
    torch.cuda.synchronize()
    got, how = out.cpu().numpy(), plan.plan()
    assert got.dtype == np.uint8 and got.shape == (frames_np.shape[0], plan.frame_bytes) and plan.frame_bytes == model.sizes(size[0], size[1], fmt)
    plan.close()
    return got, how


def _packed(frames_np, fmt, matrix="bt601", rng="tv"):
    return np.stack([model.pack(f, fmt, matrix, rng) for f in frames_np])


def _same(got, exp, what):
    bad = int((_bits(got) != _bits(exp)).sum())
    assert bad == 0, (what, bad)


# ---- both directions: frames equal the model ----

@pytest.mark.parametrize("force_general", [False, True], ids=["default", "general"])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_source_frames_equal_the_model(size, fmt, force_general):
    """One pixel, odd sizes, one lane, widths that are and are not a multiple of 8, more than one thread block with a ragged last one:
    random 10-bit samples, a binary 0 / 1023 frame and the palette frame as one batch of three.  The plan names `vec` exactly where
    w % 8 == 0."""
    packed, exp = _frames(size, fmt)
    got, how = _unpack(packed, size, fmt, force_general)
    _same(got, exp, (size, fmt, how))
    assert how == {"unpack444": _name("unpack", fmt, size[1] % 8 == 0 and not force_general), "frames": "3"}, how


@pytest.mark.parametrize("force_general", [False, True], ids=["default", "general"])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_egress_frames_equal_the_model(size, fmt, force_general):
    """The model's halves of the three images (quarter codes, both clamps' ends among them) as one batch of three; the bits outside a
    sample are written as 0."""
    _, halves = _frames(size, fmt)
    got, how = _egress(halves, fmt, force_general)
    _same(got, _packed(halves, fmt), (size, fmt, how))
    assert how == {"egress444": _name("egress", fmt, size[1] % 8 == 0 and not force_general), "frames": "3"}, how
    if fmt == "x2rgb10le":
        assert not (np.ascontiguousarray(got).view("<u4") >> 30).any()
    else:
        assert not (_bits(got) >> 10).any()


@pytest.mark.parametrize("matrix,rng", model.CASES)
@pytest.mark.parametrize("size", [(37, 131), (16, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_matrix_and_range(size, matrix, rng):
    """yuv444p10le under each of the four tables, both directions; the two RGB formats give the bytes of the defaults whatever the
    keywords say."""
    packed, _ = _frames(size, "yuv444p10le", seed=7)
    exp = np.stack([model.unpack(p, size[0], size[1], "yuv444p10le", matrix, rng) for p in packed])
    got, how = _unpack(packed, size, "yuv444p10le", matrix=matrix, rng=rng)
    _same(got, exp, (size, matrix, rng, how))
    back, how = _egress(exp, "yuv444p10le", matrix=matrix, rng=rng)
    _same(back, _packed(exp, "yuv444p10le", matrix, rng), (size, matrix, rng, how))
    assert float(exp.min()) == 0.0 and float(exp.max()) == 255.0
    for fmt in ("gbrp10le", "x2rgb10le"):
        p, e = _frames(size, fmt, seed=7)
        got, _ = _unpack(p, size, fmt, matrix=matrix, rng=rng)
        _same(got, e, (size, fmt, matrix, rng))
        back, _ = _egress(e, fmt, matrix=matrix, rng=rng)
        _same(back, _packed(e, fmt), (size, fmt, matrix, rng))


@pytest.mark.parametrize("force_general", [False, True], ids=["vec", "general"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_source_of_every_code_with_random_ignored_bits(fmt, force_general):
    """A 3 x 1024 x 8 batch: channel j of frame j runs through all 1024 codes (one per row) while the other two hold random samples, and
    the bits outside the samples — the top six of a planar word, the top two of a packed one — are random.  The halves are those of the
    clean frames."""
    h, w, n = 1024, 8, 3
    rng = np.random.default_rng(11)
    P = rng.integers(0, 1024, (n, 3, h, w), dtype=np.int64)
    for j in range(3):
        P[j, j] = np.arange(1024)[:, None]
    clean = np.stack([model.pack_samples(p, fmt) for p in P])
    if fmt == "x2rgb10le":
        dirty = (clean.view("<u4") | (rng.integers(0, 4, clean.size // 4, dtype=np.uint32).reshape(n, -1) << 30)).view(np.uint8)
    else:
        dirty = (clean.view("<u2") | (rng.integers(0, 64, clean.size // 2, dtype=np.uint16).reshape(n, -1) << 10)).view(np.uint8)
    assert dirty.shape == clean.shape and not np.array_equal(dirty, clean)
    exp = np.stack([model.unpack(p, h, w, fmt) for p in clean])
    got, how = _unpack(dirty, (h, w), fmt, force_general)
    assert how["unpack444"] == _name("unpack", fmt, not force_general)
    _same(got, exp, (fmt, how))


@pytest.mark.parametrize("force_general", [False, True], ids=["vec", "general"])
def test_egress_of_every_half_bit_pattern(force_general):
    """A 256 x 256 frame whose channel values run through all 65 536 half bit patterns (NaNs of both kinds, infinities, negatives, -0,
    subnormals and every tie of the quantiser), each channel in another order: equal to the model bit for bit, both layouts."""
    h = w = 256
    pat = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    frame = np.stack([pat, pat[::-1], np.roll(pat, 12345)], axis=-1).view(np.float16).reshape(1, h, w, 3)
    for c in range(3):
        assert len(set(frame[0, :, :, c].view(np.uint16).reshape(-1).tolist())) == 65536
    for fmt in ("yuv444p10le", "x2rgb10le"):
        got, how = _egress(frame, fmt, force_general)
        assert how["egress444"] == _name("egress", fmt, not force_general)
        _same(got, _packed(frame, fmt), (fmt, how))
    # grey pixels under the RGB scale: every field is (65729 q + 32768) >> 16 of the quantiser's q, which pins it for every half
    grey = np.repeat(pat[:, None], 3, axis=1).view(np.float16).reshape(1, h, w, 3)
    want = (65729 * model.quantise(grey[0, :, :, 0]) + 32768) >> 16
    got, _ = _egress(grey, "gbrp10le", force_general)
    planes = _bits(got).reshape(3, h, w).astype(np.int64)
    assert all(int((planes[j] != want).sum()) == 0 for j in range(3)) and len(set(want.reshape(-1).tolist())) == 1021


# ---- strided batches ----

# (source offset, destination offset, source padding, destination padding, vec) in bytes
STRIDES = [(0, 0, 8, 12, True), (4, 8, 4, 4, True), (0, 0, 4, 6, False), (0, 0, 6, 4, False), (0, 0, 2, 2, False)]


@pytest.mark.parametrize("kind", ["unpack", "egress"])
@pytest.mark.parametrize("fmt", ["yuv444p10le", "x2rgb10le"])
def test_strided_batches_leave_the_padding_alone(kind, fmt):
    """n = 3 frames (19 x 40) that are slices of bigger buffers on both sides, frame strides larger than a frame.  Strides that are
    multiples of 4 allow `vec`; one that is not takes `general` — where the 10-bit side is x2rgb10le such a stride is refused there.  A
    base that is a multiple of 2 but not of 4 takes `general` for planar and is refused for x2rgb10le.  Every frame right, every sentinel
    byte outside the frames untouched."""
    import torch
    from pythoncrt_amd import EgressDeep444, UnpackDeep444
    from pythoncrt_amd._lib import CrtfxError
    size, n = (19, 40), 3
    pbytes, rbytes = model.sizes(size[0], size[1], fmt), size[0] * size[1] * 6
    rng = np.random.default_rng(3)
    if kind == "unpack":
        src = np.stack([model.pack_samples(rng.integers(0, 1024, (3,) + size), fmt) for _ in range(n)])
        exp = np.stack([model.unpack(p, size[0], size[1], fmt) for p in src]).view(np.uint8).reshape(n, rbytes)
        sbytes, dbytes = pbytes, rbytes
    else:
        src = rng.integers(0, 65536, (n, rbytes // 2), dtype=np.uint16).view(np.uint8).reshape(n, rbytes)
        exp = _packed(src.view(np.float16).reshape((n,) + size + (3,)), fmt)
        sbytes, dbytes = rbytes, pbytes
    cases = list(STRIDES)
    cases += [(2, 0, 2, 4, False), (0, 2, 4, 2, False)]                                     # a base that is a multiple of 2 only, on either side
    for s_off, d_off, s_pad, d_pad, vec in cases:
        deep_off, deep_pad = (s_off, s_pad) if kind == "unpack" else (d_off, d_pad)
        refused = fmt == "x2rgb10le" and (deep_off % 4 != 0 or deep_pad % 4 != 0)
        sbuf = torch.full((s_off + n * (sbytes + s_pad) + 16,), 0xEE, dtype=torch.uint8, device=_dev())
        dbuf = torch.full((d_off + n * (dbytes + d_pad) + 16,), 0x5A, dtype=torch.uint8, device=_dev())
        assert sbuf.data_ptr() % 4 == 0 and dbuf.data_ptr() % 4 == 0
        sview = sbuf[s_off:s_off + n * (sbytes + s_pad)].view(n, sbytes + s_pad)[:, :sbytes]
        dview = dbuf[d_off:d_off + n * (dbytes + d_pad)].view(n, dbytes + d_pad)[:, :dbytes]
        sview.copy_(torch.from_numpy(src).to(_dev()))
        plan = (UnpackDeep444 if kind == "unpack" else EgressDeep444)(_dev(), size, layout=fmt)

        def go():
            if kind == "unpack":
                out = dview.view(torch.float16).unflatten(1, size + (3,))
                assert plan.run(sview, out=out) is out
            else:
                assert plan.run(sview.view(torch.float16).unflatten(1, size + (3,)), out=dview) is dview
        if refused:
            with pytest.raises(CrtfxError) as e:
                go()
            assert e.value.code == _lib.E_INVALID and "multiple of 4" in str(e.value)
            torch.cuda.synchronize()
            assert bool((dbuf == 0x5A).all())
        else:
            go()
            torch.cuda.synchronize()
            assert plan.plan() == {f"{kind}444": _name(kind, fmt, vec), "frames": "3"}, (plan.plan(), s_off, d_off, s_pad, d_pad)
            assert np.array_equal(dview.cpu().numpy(), exp), (kind, fmt, s_off, d_off, s_pad, d_pad)
            keep = torch.ones_like(dbuf, dtype=torch.bool)
            keep[d_off:d_off + n * (dbytes + d_pad)].view(n, dbytes + d_pad)[:, :dbytes] = False
            assert bool((dbuf[keep] == 0x5A).all()), (kind, fmt, s_off, d_off)
        plan.close()


# ---- bad arguments ----

@pytest.mark.parametrize("kind", ["unpack", "egress"])
@pytest.mark.parametrize("fmt", ["gbrp10le", "x2rgb10le"])
def test_bad_arguments_return_the_stated_codes(kind, fmt):
    import torch
    from pythoncrt_amd import EgressDeep444, UnpackDeep444
    from pythoncrt_amd._lib import CrtfxError
    cls = UnpackDeep444 if kind == "unpack" else EgressDeep444
    with pytest.raises(CrtfxError) as e:
        cls(_dev(), (8, 8), layout=fmt, pix_fmt=_lib.PIX_U8)
    assert e.value.code == _lib.E_UNSUPPORTED and "half" in str(e.value)
    with pytest.raises(CrtfxError) as e:
        cls(_dev(), (0, 16), layout=fmt)
    assert e.value.code == _lib.E_INVALID
    for bad in ("yuv444p", "p010le", "planar"):
        with pytest.raises(ValueError):
            cls(_dev(), (8, 8), layout=bad)
    plan = cls(_dev(), (8, 8), layout=fmt)
    pb = 256 if fmt == "x2rgb10le" else 384
    assert plan.frame_bytes == pb and plan.plan() == {f"{kind}444": _name(kind, fmt, True), "frames": "0"}
    packed = torch.zeros((2, pb), dtype=torch.uint8, device=_dev())
    rgb = torch.zeros((2, 8, 8, 3), dtype=torch.float16, device=_dev())
    src, dst = (packed, rgb) if kind == "unpack" else (rgb, packed)
    sbytes, dbytes = (pb, 384) if kind == "unpack" else (384, pb)
    with pytest.raises(CrtfxError) as e:
        plan.run(dst)                                                                           # the other side's dtype
    assert e.value.code == _lib.E_UNSUPPORTED
    with pytest.raises(ValueError):
        plan.run(src[:, :-2] if kind == "unpack" else src[:, :, :-1])                           # a wrong shape
    with pytest.raises(ValueError):
        plan.run(src, out=dst[:1])
    assert int(plan.run(src[:0]).shape[0]) == 0
    with pytest.raises(CrtfxError) as e:
        plan.set_option(99, 1)
    assert e.value.code == _lib.E_INVALID and "option" in str(e.value)
    with pytest.raises(CrtfxError) as e:
        plan.set_option(1, 2)
    assert e.value.code == _lib.E_INVALID and "FORCE_GENERAL" in str(e.value)
    lib = plan.lib
    run, err = getattr(lib, f"crtfx_{kind}444_run"), getattr(lib, f"crtfx_{kind}444_last_error")
    st = torch.cuda.current_stream().cuda_stream
    dst.fill_(0)
    sp, dp = src.data_ptr(), dst.data_ptr()
    assert run(plan._plan, sp, sbytes, dp, dbytes, 0, st) == _lib.E_INVALID and b"n = 0" in err(plan._plan)
    assert run(plan._plan, None, sbytes, dp, dbytes, 1, st) == _lib.E_INVALID and b"null" in err(plan._plan)
    assert run(plan._plan, sp, sbytes, None, dbytes, 1, st) == _lib.E_INVALID
    word = b"multiple of 4" if fmt == "x2rgb10le" else b"odd"
    deep_first = kind == "unpack"                                                               # which side is the 10-bit one
    assert run(plan._plan, sp + 1, sbytes, dp, dbytes, 1, st) == _lib.E_INVALID and (word if deep_first else b"odd") in err(plan._plan)
    assert run(plan._plan, sp, sbytes, dp + 1, dbytes, 1, st) == _lib.E_INVALID and (b"odd" if deep_first else word) in err(plan._plan)
    assert run(plan._plan, sp, sbytes + 1, dp, dbytes, 2, st) == _lib.E_INVALID and (word if deep_first else b"odd") in err(plan._plan)
    assert run(plan._plan, sp, sbytes, dp, dbytes + 1, 2, st) == _lib.E_INVALID and (b"odd" if deep_first else word) in err(plan._plan)
    if fmt == "x2rgb10le":                                                                      # even is not enough on the packed side
        assert run(plan._plan, sp + (2 if deep_first else 0), sbytes, dp + (0 if deep_first else 2), dbytes, 1, st) == _lib.E_INVALID
        assert b"multiple of 4" in err(plan._plan)
    assert run(plan._plan, sp, sbytes - 4, dp, dbytes, 2, st) == _lib.E_INVALID and b"strides" in err(plan._plan)  # a stride below a frame
    assert run(plan._plan, sp, sbytes, dp, dbytes - 4, 2, st) == _lib.E_INVALID and b"strides" in err(plan._plan)
    torch.cuda.synchronize()
    assert int(dst.view(torch.uint8).sum()) == 0                                                # no refused call wrote anything
    plan.close()


# ---- a 1080p batch ----

def test_a_1080p_batch():
    """Two 1080 x 1920 frames through both directions of both layouts on the default (vec) path."""
    size = (1080, 1920)
    P = np.random.default_rng(8).integers(0, 1024, (2, 3) + size, dtype=np.int64)
    for fmt in ("yuv444p10le", "x2rgb10le"):
        packed = np.stack([model.pack_samples(p, fmt) for p in P])
        exp = np.stack([model.unpack(p, size[0], size[1], fmt) for p in packed])
        got, how = _unpack(packed, size, fmt)
        assert how == {"unpack444": _name("unpack", fmt, True), "frames": "2"}
        _same(got, exp, (fmt, how))
        back, how = _egress(exp, fmt)
        assert how == {"egress444": _name("egress", fmt, True), "frames": "2"}
        _same(back, _packed(exp, fmt), (fmt, how))


# ---- process_frames and the CLI ----

def _unpack_any(p, h, w, fmt, **mkw):
    return model.unpack(p, h, w, fmt, **mkw) if fmt in model.FORMATS else deep_model.unpack(p, h, w, fmt, **mkw)


def _pack_any(f, fmt, **mkw):
    return model.pack(f, fmt, **mkw) if fmt in model.FORMATS else deep_model.pack(f, fmt, **mkw)


def _bytes_any(h, w, fmt):
    return model.sizes(h, w, fmt) if fmt in model.FORMATS else deep_model.sizes(h, w)[2]


def _source_any(rng, n, h, w, fmt):
    """n random packed frames of `fmt`: uint8 [n, frame_bytes]."""
    if fmt in model.FORMATS:
        return np.stack([model.pack_samples(rng.integers(0, 1024, (3, h, w)), fmt) for _ in range(n)])
    fb = deep_model.sizes(h, w)[2]
    return deep_model.to_bytes(rng.integers(0, 1024, (n, fb // 2)).astype(np.uint16) << (6 if fmt == "p010le" else 0)).reshape(n, fb)


def _expected_render(src, size, in_fmt, out_fmt, settings, seed, batch, in_kw=None, out_kw=None):
    """model.pack(FramePipeline(dtype=float16, same settings and seed).run(model.unpack(src))), in batches of `batch` frames with the state
    carried from one to the next as the render loops do: uint8 [n, frame_bytes]."""
    import torch
    from pythoncrt_amd.pipeline import FramePipeline
    h, w = size
    rgb = torch.from_numpy(np.stack([_unpack_any(p, h, w, in_fmt, **(in_kw or {})) for p in src])).to(_dev())
    pipe = FramePipeline(_dev(), h, w, settings, fps=30.0, noise_seed=seed, dtype=torch.float16)
    outs, state = [], None
    for lo in range(0, len(src), batch):
        out, state = pipe.run(rgb[lo:lo + batch], first_index=lo, state=state)
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    res = np.concatenate(outs)
    assert res.dtype == np.float16
    return np.stack([_pack_any(f, out_fmt, **(out_kw or {})) for f in res])


PAIRS = [("yuv444p10le", "gbrp10le"), ("x2rgb10le", "yuv444p10le"), ("gbrp10le", "x2rgb10le"), ("p010le", "x2rgb10le"), ("yuv444p10le", "p010le")]


@pytest.mark.parametrize("in_fmt,out_fmt", PAIRS)
@pytest.mark.parametrize("config", ["defaults", "baseline5"])
def test_process_frames_runs_the_new_formats_on_both_ends(config, in_fmt, out_fmt):
    """Four 72 x 320 frames in one batch, the new formats on both ends and mixed with p010le, the grain fixed by noise_seed: what the
    writer gets equals the model's bytes of a half FramePipeline run on the model's halves, byte for byte — with the defaults, and with
    BASELINE config 5's settings (its size aside)."""
    import pythoncrt_amd as pc
    from pythoncrt_amd.pipeline import RenderSettings, baseline_config
    h, w, n = 72, 320, 4
    rs = RenderSettings() if config == "defaults" else baseline_config(5)[0]
    kw = {} if config == "defaults" else dataclasses.asdict(rs)
    src = _source_any(np.random.default_rng(44), n, h, w, in_fmt)
    fb_in, fb_out = _bytes_any(h, w, in_fmt), _bytes_any(h, w, out_fmt)
    wide = "<u4" if in_fmt == "x2rgb10le" else "<u2"
    items = [src[0], src[1].reshape(2, -1), src[2].view(wide), src[3]]                # any shape; 16-bit / 32-bit words are taken too
    got = []
    wrote = pc.process_frames(iter(items), lambda a: got.append(np.array(a)), w, h, 30.0, n, noise_seed=9, batch=4,
                              in_pix_fmt=in_fmt, out_pix_fmt=out_fmt, **kw)
    assert wrote == n and src.shape == (n, fb_in) and all(a.shape == (fb_out,) and a.dtype == np.uint8 for a in got)
    exp = _expected_render(src, (h, w), in_fmt, out_fmt, rs, 9, 4)
    for i in range(n):
        assert np.array_equal(got[i], exp[i]), (config, in_fmt, out_fmt, i, int((got[i] != exp[i]).sum()))
    assert not np.array_equal(got[0], got[1])


def test_process_frames_refuses_without_reading_a_frame():
    import pythoncrt_amd as pc

    def never():
        raise AssertionError("a frame was read")
        yield

    for kw, word in ((dict(in_pix_fmt="gbrp10le"), "one end"), (dict(out_pix_fmt="x2rgb10le", in_pix_fmt="nv12"), "one end"),
                     (dict(in_pix_fmt="yuv444p10le", out_pix_fmt="p010le", in_size=(36, 160)), "in_size"),
                     (dict(in_pix_fmt="x2rgb10le", out_pix_fmt="gbrp10le", resize_on="host"), "host")):
        with pytest.raises(ValueError) as e:
            pc.process_frames(never(), lambda a: None, 320, 72, 30.0, 1, **kw)
        assert word in str(e.value), (kw, str(e.value))
    fb = model.sizes(72, 320, "gbrp10le")
    with pytest.raises(ValueError) as e:                                                       # an x2rgb10le frame where a planar one is due
        pc.process_frames(iter([np.zeros(fb * 2 // 3, dtype=np.uint8)]), lambda a: None, 320, 72, 30.0, 1, in_pix_fmt="gbrp10le", out_pix_fmt="gbrp10le")
    assert str(fb) in str(e.value) and str(fb * 2 // 3) in str(e.value)


@pytest.mark.parametrize("io", ["staged", "mapped"])
@pytest.mark.parametrize("in_fmt,out_fmt", [("yuv444p10le", "x2rgb10le"), ("p010le", "gbrp10le"), ("x2rgb10le", "p010le")])
def test_cli_with_the_new_formats(tmp_path, io, in_fmt, out_fmt):
    """A 3-frame 64 x 96 file (batch 2: a full batch and a short one), --io staged and --io mapped, bt709 on both ends: the output file is
    the model's — the first batch of two, then the third frame on the state the first batch left."""
    from pythoncrt_amd import cli
    from pythoncrt_amd.pipeline import RenderSettings
    n, h, w = 3, 64, 96
    src = _source_any(np.random.default_rng(45), n, h, w, in_fmt)
    (tmp_path / "in.raw").write_bytes(src.tobytes())
    flags = ["--width", str(w), "--height", str(h), "--fps", "30", "--batch", "2", "--noise-seed", "17", "--persistence", "0.3", "--io", io,
             "--in-pix-fmt", in_fmt, "--out-pix-fmt", out_fmt, "--in-matrix", "bt709", "--out-matrix", "bt709", "--out-range", "pc"]
    assert cli.main(flags + ["--input", str(tmp_path / "in.raw"), "--output", str(tmp_path / "out.raw")]) == 0
    got = np.frombuffer((tmp_path / "out.raw").read_bytes(), dtype=np.uint8)
    fb = _bytes_any(h, w, out_fmt)
    assert got.size == n * fb
    in_kw = {} if in_fmt in model.ORDER else dict(matrix="bt709")
    out_kw = {} if out_fmt in model.ORDER else dict(matrix="bt709", rng="pc")
    want = _expected_render(src, (h, w), in_fmt, out_fmt, RenderSettings(persistence=0.3), 17, 2, in_kw, out_kw)
    for i in range(n):
        assert np.array_equal(got.reshape(n, fb)[i], want[i]), (io, i, int((got.reshape(n, fb)[i] != want[i]).sum()))


def test_cli_through_pipes(tmp_path):
    """stdin -> stdout in a child process (`--input - --output -`): gbrp10le in, yuv444p10le out, the bytes of the file run."""
    import subprocess
    import sys
    from pythoncrt_amd import cli
    n, h, w = 3, 64, 96
    src = _source_any(np.random.default_rng(46), n, h, w, "gbrp10le")
    (tmp_path / "in.raw").write_bytes(src.tobytes())
    flags = ["--width", str(w), "--height", str(h), "--fps", "30", "--batch", "2", "--noise-seed", "5", "--in-pix-fmt", "gbrp10le",
             "--out-pix-fmt", "yuv444p10le"]
    assert cli.main(flags + ["--input", str(tmp_path / "in.raw"), "--output", str(tmp_path / "out.raw")]) == 0
    r = subprocess.run([sys.executable, "-m", "pythoncrt_amd.cli", *flags, "--input", "-", "--output", "-"], input=src.tobytes(), capture_output=True,
                       cwd=_lib.ROOT, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout == (tmp_path / "out.raw").read_bytes() and len(r.stdout) == n * model.sizes(h, w, "yuv444p10le")
