"""The 10-bit pair on the GPU: UnpackYuv10 (k_unpack10_420) and EgressYuv10 (k_egress10_420), vec and general path, yuv420p10le and p010le,
against the integer host model of tests/deep_model.py — equality means zero differing bits, halves compared as their uint16 patterns — and
process_frames / the CLI with 10-bit formats on both ends against the model around a half FramePipeline."""
import dataclasses

import numpy as np
import pytest

from pythoncrt_amd import _lib
from tests import deep_model as model

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (2, 2), (3, 5), (16, 64), (34, 132), (37, 131), (270, 480)]
LAYOUTS = list(model.LAYOUTS)


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _name(kind, layout, vec):
    return f"k_{kind}10_420<{layout},{'vec' if vec else 'general'}>"


def _bits(a):
    """The uint16 patterns of a float16 array / the uint16 words of a packed uint8 one."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint16)


_CACHE = {}


def _frames(size, layout, seed=0):
    """The three packed test frames of a size in `layout`, uint8 [3, frame_bytes], and the model's halves of them under bt601 / tv
    (computed once per size and seed: the samples are the same in both layouts)."""
    key = (size, seed)
    if key not in _CACHE:
        imgs = model.images(*size, seed=seed)
        _CACHE[key] = (imgs, np.stack([model.unpack(p, size[0], size[1]) for p in imgs]))
    imgs, halves = _CACHE[key]
    return np.stack([model.relayout(p, size[0], size[1], layout) for p in imgs]), halves


def _unpack(packed_np, size, layout, force_general=False, matrix="bt601", rng="tv"):
    """(float16[n, h, w, 3] from the device, the plan's words) for a stack of packed frames."""
    import torch
    from pythoncrt_amd import UnpackYuv10
    plan = UnpackYuv10(_dev(), size, layout=layout, matrix=matrix, range=rng)
    if force_general:
        plan.set_option(_lib.UNPACK10_OPT_FORCE_GENERAL, 1)
    out = plan.run(torch.from_numpy(packed_np).to(_dev()))
    torch.cuda.synchronize()
    got, how = out.cpu().numpy(), plan.plan()
    assert got.dtype == np.float16 and got.shape == (packed_np.shape[0],) + tuple(size) + (3,)
    plan.close()
    return got, how


def _egress(frames_np, layout, force_general=False, matrix="bt601", rng="tv"):
    """(uint8[n, frame_bytes] from the device, the plan's words) for a stack of float16 frames."""
    import torch
    from pythoncrt_amd import EgressYuv10
    size = tuple(frames_np.shape[1:3])
    plan = EgressYuv10(_dev(), size, layout=layout, matrix=matrix, range=rng)
    if force_general:
        plan.set_option(_lib.EGRESS10_OPT_FORCE_GENERAL, 1)
    out = plan.run(torch.from_numpy(frames_np).to(_dev()))
    torch.cuda.synchronize()
    got, how = out.cpu().numpy(), plan.plan()
    assert got.dtype == np.uint8 and got.shape == (frames_np.shape[0], plan.frame_bytes) and plan.frame_bytes == model.sizes(*size)[2]
    plan.close()
    return got, how


def _packed(frames_np, layout, matrix="bt601", rng="tv"):
    return np.stack([model.pack(f, layout, matrix, rng) for f in frames_np])


def _same_halves(got, exp, what):
    bad = int((_bits(got) != _bits(exp)).sum())
    assert bad == 0, (what, bad)


def _same_words(got, exp, what):
    bad = int((_bits(got) != _bits(exp)).sum())
    assert bad == 0, (what, bad)


# ---- both directions: frames equal the model --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("force_general", [False, True], ids=["default", "general"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_source_frames_equal_the_model(size, layout, force_general):
    """One pixel, one block, odd sizes, widths that are and are not a multiple of 8, more than one thread block: random 10-bit samples, a
    binary 0 / 1023 frame and the palette frame as one batch of three.  The plan names `vec` exactly where w % 8 == 0."""
    packed, exp = _frames(size, layout)
    got, how = _unpack(packed, size, layout, force_general)
    _same_halves(got, exp, (size, layout, how))
    assert how == {"unpack10": _name("unpack", layout, size[1] % 8 == 0 and not force_general), "frames": "3"}, how


@pytest.mark.parametrize("force_general", [False, True], ids=["default", "general"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_egress_frames_equal_the_model(size, layout, force_general):
    """The model's halves of the three images (quarter codes, both clamps' ends among them) and a fourth frame of random half bit patterns
    (fractions, negatives, NaNs, infinities), as one batch of four."""
    _, halves = _frames(size, layout)
    noise = np.random.default_rng(size[0] * 1000 + size[1]).integers(0, 65536, halves.shape[1:], dtype=np.uint16).view(np.float16)
    frames = np.concatenate([halves, noise[None]])
    got, how = _egress(frames, layout, force_general)
    _same_words(got, _packed(frames, layout), (size, layout, how))
    assert how == {"egress10": _name("egress", layout, size[1] % 8 == 0 and not force_general), "frames": "4"}, how


@pytest.mark.parametrize("matrix,rng", model.CASES)
@pytest.mark.parametrize("size", [(37, 131), (16, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_matrix_and_range(size, matrix, rng):
    for layout in LAYOUTS:
        packed, _ = _frames(size, layout, seed=7)
        exp = np.stack([model.unpack(p, size[0], size[1], layout, matrix, rng) for p in packed])
        got, how = _unpack(packed, size, layout, matrix=matrix, rng=rng)
        _same_halves(got, exp, (size, layout, matrix, rng, how))
        back, how = _egress(exp, layout, matrix=matrix, rng=rng)
        _same_words(back, _packed(exp, layout, matrix, rng), (size, layout, matrix, rng, how))
    assert float(exp.min()) == 0.0 and float(exp.max()) == 255.0


@pytest.mark.parametrize("force_general", [False, True], ids=["default", "general"])
def test_source_ignores_the_bits_outside_the_sample(force_general):
    """yuv420p10le words with their high six bits set and p010le words with their low six bits set give the halves of the clean frames."""
    for size in ((37, 131), (16, 64)):
        for layout, junk in (("yuv420p10le", 0xFC00), ("p010le", 0x003F)):
            packed, exp = _frames(size, layout)
            dirty = model.to_bytes(model.words(packed) | np.uint16(junk))
            assert dirty.shape == packed.shape and not np.array_equal(dirty, packed)
            got, how = _unpack(dirty, size, layout, force_general)
            _same_halves(got, exp, (size, layout, how))


# ---- egress: all 65 536 half bit patterns -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("force_general", [False, True], ids=["vec", "general"])
def test_egress_of_every_half_bit_pattern(force_general):
    """144 x 160 x 3 = 69 120 samples: sample i of the flat half array has pattern i mod 65536, a second frame has them in reversed order
    (so chroma sums mix): NaNs of both kinds, infinities, negatives, -0, subnormals and every tie of the quantiser.  Equal to the model
    bit for bit, both layouts."""
    h, w = 144, 160
    pat = (np.arange(h * w * 3, dtype=np.int64) % 65536).astype(np.uint16)
    frames = np.stack([pat, pat[::-1]]).view(np.float16).reshape(2, h, w, 3)
    assert len(set(frames[0].view(np.uint16).reshape(-1).tolist())) == 65536
    for layout in LAYOUTS:
        got, how = _egress(frames, layout, force_general)
        assert how["egress10"] == _name("egress", layout, not force_general)
        _same_words(got, _packed(frames, layout), (layout, how))


@pytest.mark.parametrize("force_general", [False, True], ids=["vec", "general"])
def test_full_range_grey_pins_the_quantiser(force_general):
    """Grey pixels (one bit pattern in R, G and B; pixel p of a batch of three 144 x 160 frames has pattern p mod 65536, so every pattern
    occurs) under the full-range matrix: the Y row sums to 65729 = floor(1023/1020 * 65536 + 0.5), so Y = (65729 q + 32768) >> 16 — q itself
    below q = 170 and an injective function of q throughout (1021 values) — which pins q = rint_to_even(min(max(4 f, 0), 1020)), NaN -> 0,
    for every half f, the matrix aside."""
    h, w, n = 144, 160, 3
    pat = (np.arange(n * h * w, dtype=np.int64) % 65536).astype(np.uint16)
    frames = np.repeat(pat[:, None], 3, axis=1).view(np.float16).reshape(n, h, w, 3)
    q = model.quantise(frames[..., 0])
    want = (65729 * q + 32768) >> 16
    assert len(set(want.reshape(-1).tolist())) == 1021 and np.array_equal(want[q < 170], q[q < 170]) and want.max() == 1023
    for matrix in ("bt601", "bt709"):
        assert sum(model.YUV_MATRICES[(matrix, "pc")][0]) == 65729
        got, _ = _egress(frames, "yuv420p10le", force_general, matrix=matrix, rng="pc")
        y = model.words(got)[:, :h * w].reshape(n, h, w).astype(np.int64)
        assert int((y != want).sum()) == 0, (matrix, int((y != want).sum()))


# ---- strided batches ----------------------------------------------------------------------------------------------------------------------

STRIDES = [(0, 0, 8, 12, True), (4, 8, 4, 4, True), (2, 0, 4, 4, False), (0, 2, 4, 4, False), (0, 0, 2, 4, False), (0, 0, 4, 6, False), (6, 2, 2, 2, False)]


@pytest.mark.parametrize("kind", ["unpack", "egress"])
def test_strided_batches_leave_the_padding_alone(kind):
    """n = 3 frames (19 x 40: an odd height under the vec path) that are slices of bigger buffers on both sides, frame strides larger than a
    frame.  A base that is misaligned by 2, or a stride that is no multiple of 4, takes `general`; multiples of 4 allow `vec`.  Every frame
    right and the same in both paths, every sentinel byte outside the frames untouched."""
    import torch
    from pythoncrt_amd import EgressYuv10, UnpackYuv10
    size, n = (19, 40), 3
    ybytes, rbytes = model.sizes(*size)[2], size[0] * size[1] * 6
    rng = np.random.default_rng(3)
    for layout in LAYOUTS:
        if kind == "unpack":
            src = model.to_bytes(rng.integers(0, 1024, (n, ybytes // 2)).astype(np.uint16) << (6 if layout == "p010le" else 0)).reshape(n, ybytes)
            exp = np.stack([model.unpack(p, size[0], size[1], layout) for p in src]).view(np.uint8).reshape(n, rbytes)
            sbytes, dbytes = ybytes, rbytes
        else:
            src = rng.integers(0, 65536, (n, rbytes // 2), dtype=np.uint16).view(np.uint8).reshape(n, rbytes)
            exp = _packed(src.view(np.float16).reshape((n,) + size + (3,)), layout)
            sbytes, dbytes = rbytes, ybytes
        for s_off, d_off, s_pad, d_pad, vec in STRIDES:
            sbuf = torch.full((s_off + n * (sbytes + s_pad) + 16,), 0xEE, dtype=torch.uint8, device=_dev())
            dbuf = torch.full((d_off + n * (dbytes + d_pad) + 16,), 0x5A, dtype=torch.uint8, device=_dev())
            assert sbuf.data_ptr() % 4 == 0 and dbuf.data_ptr() % 4 == 0
            sview = sbuf[s_off:s_off + n * (sbytes + s_pad)].view(n, sbytes + s_pad)[:, :sbytes]
            dview = dbuf[d_off:d_off + n * (dbytes + d_pad)].view(n, dbytes + d_pad)[:, :dbytes]
            sview.copy_(torch.from_numpy(src).to(_dev()))
            if kind == "unpack":
                plan = UnpackYuv10(_dev(), size, layout=layout)
                out = dview.view(torch.float16).unflatten(1, size + (3,))
                assert plan.run(sview, out=out) is out
            else:
                plan = EgressYuv10(_dev(), size, layout=layout)
                assert plan.run(sview.view(torch.float16).unflatten(1, size + (3,)), out=dview) is dview
            torch.cuda.synchronize()
            assert plan.plan() == {f"{kind}10": _name(kind, layout, vec), "frames": "3"}, (plan.plan(), s_off, d_off, s_pad, d_pad)
            assert np.array_equal(dview.cpu().numpy(), exp), (kind, layout, s_off, d_off, s_pad, d_pad)
            keep = torch.ones_like(dbuf, dtype=torch.bool)
            keep[d_off:d_off + n * (dbytes + d_pad)].view(n, dbytes + d_pad)[:, :dbytes] = False
            assert bool((dbuf[keep] == 0x5A).all()), (kind, layout, s_off, d_off)
            y, *_ = plan.planes(sview if kind == "unpack" else dview)
            assert tuple(y.shape) == (n,) + size and y.dtype == torch.int16
            plan.close()


# ---- bad arguments ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["unpack", "egress"])
def test_bad_arguments_return_the_stated_codes(kind):
    import torch
    from pythoncrt_amd import EgressYuv10, UnpackYuv10
    from pythoncrt_amd._lib import CrtfxError
    cls = UnpackYuv10 if kind == "unpack" else EgressYuv10
    with pytest.raises(CrtfxError) as e:
        cls(_dev(), (8, 8), pix_fmt=_lib.PIX_U8)
    assert e.value.code == _lib.E_UNSUPPORTED and "half" in str(e.value)
    with pytest.raises(CrtfxError) as e:
        cls(_dev(), (0, 16))
    assert e.value.code == _lib.E_INVALID
    with pytest.raises(ValueError):
        cls(_dev(), (8, 8), layout="nv12")
    plan = cls(_dev(), (8, 8))
    assert plan.frame_bytes == 192 and plan.plan() == {f"{kind}10": _name(kind, "yuv420p10le", True), "frames": "0"}
    packed = torch.zeros((2, 192), dtype=torch.uint8, device=_dev())
    rgb = torch.zeros((2, 8, 8, 3), dtype=torch.float16, device=_dev())
    src, dst = (packed, rgb) if kind == "unpack" else (rgb, packed)
    sbytes, dbytes = (192, 384) if kind == "unpack" else (384, 192)
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
    run, err = getattr(lib, f"crtfx_{kind}10_run"), getattr(lib, f"crtfx_{kind}10_last_error")
    st = torch.cuda.current_stream().cuda_stream
    dst.fill_(0)
    sp, dp = src.data_ptr(), dst.data_ptr()
    assert run(plan._plan, sp, sbytes, dp, dbytes, 0, st) == _lib.E_INVALID and b"n = 0" in err(plan._plan)
    assert run(plan._plan, None, sbytes, dp, dbytes, 1, st) == _lib.E_INVALID and b"null" in err(plan._plan)
    assert run(plan._plan, sp, sbytes, None, dbytes, 1, st) == _lib.E_INVALID
    assert run(plan._plan, sp + 1, sbytes, dp, dbytes, 1, st) == _lib.E_INVALID and b"odd" in err(plan._plan)      # an odd base
    assert run(plan._plan, sp, sbytes, dp + 1, dbytes, 1, st) == _lib.E_INVALID and b"odd" in err(plan._plan)
    assert run(plan._plan, sp, sbytes + 1, dp, dbytes, 2, st) == _lib.E_INVALID and b"odd" in err(plan._plan)      # an odd stride
    assert run(plan._plan, sp, sbytes - 2, dp, dbytes, 2, st) == _lib.E_INVALID and b"strides" in err(plan._plan)  # a stride below a frame
    assert run(plan._plan, sp, sbytes, dp, dbytes - 2, 2, st) == _lib.E_INVALID and b"strides" in err(plan._plan)
    if torch.cuda.device_count() > 1:
        with torch.cuda.device(1 if _dev().index == 0 else 0):
            assert run(plan._plan, sp, sbytes, dp, dbytes, 1, st) == _lib.E_INVALID and b"current device" in err(plan._plan)
    torch.cuda.synchronize()
    assert int(dst.view(torch.uint8).sum()) == 0                                                # no refused call wrote anything
    plan.close()


# ---- process_frames -----------------------------------------------------------------------------------------------------------------------

def _expected_render(src, size, in_fmt, out_fmt, settings, seed, batch, **mkw):
    """deep_model.pack(FramePipeline(dtype=float16, same settings and seed).run(deep_model.unpack(src))), in batches of `batch` frames with
    the state carried from one to the next as the render loops do: uint8 [n, frame_bytes]."""
    import torch
    from pythoncrt_amd.pipeline import FramePipeline
    h, w = size
    rgb = torch.from_numpy(np.stack([model.unpack(p, h, w, in_fmt) for p in src])).to(_dev())
    pipe = FramePipeline(_dev(), h, w, settings, fps=30.0, noise_seed=seed, dtype=torch.float16)
    outs, state = [], None
    for lo in range(0, len(src), batch):
        out, state = pipe.run(rgb[lo:lo + batch], first_index=lo, state=state)
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    res = np.concatenate(outs)
    assert res.dtype == np.float16
    return np.stack([model.pack(f, out_fmt, **mkw) for f in res])


@pytest.mark.parametrize("config", ["defaults", "baseline5"])
def test_process_frames_runs_ten_bit_on_both_ends(config):
    """Four 72 x 320 frames in one batch, p010le in and yuv420p10le out (and the other way round), the grain fixed by noise_seed: what the
    writer gets equals the model's bytes of a half FramePipeline run on the model's halves, byte for byte — with the defaults, and with
    BASELINE config 5's settings (its size aside)."""
    import pythoncrt_amd as pc
    from pythoncrt_amd.pipeline import RenderSettings, baseline_config
    h, w, n = 72, 320, 4
    rs = RenderSettings() if config == "defaults" else baseline_config(5)[0]
    kw = {} if config == "defaults" else dataclasses.asdict(rs)
    fb = model.sizes(h, w)[2]
    samples = np.random.default_rng(44).integers(0, 1024, (n, fb // 2)).astype(np.uint16)
    for in_fmt, out_fmt in (("p010le", "yuv420p10le"), ("yuv420p10le", "p010le")):
        src = model.to_bytes(samples << (6 if in_fmt == "p010le" else 0)).reshape(n, fb)
        got = []
        items = [src[0], src[1].reshape(2, -1), model.words(src[2]), src[3]]             # any shape; 16-bit words are taken too
        wrote = pc.process_frames(iter(items), lambda a: got.append(np.array(a)), w, h, 30.0, n, noise_seed=9, batch=4,
                                  in_pix_fmt=in_fmt, out_pix_fmt=out_fmt, **kw)
        assert wrote == n and all(a.shape == (fb,) and a.dtype == np.uint8 for a in got)
        exp = _expected_render(src, (h, w), in_fmt, out_fmt, rs, 9, 4)
        for i in range(n):
            assert np.array_equal(got[i], exp[i]), (config, in_fmt, i, int((got[i] != exp[i]).sum()))
        assert not np.array_equal(got[0], got[1])


def test_process_frames_refuses_without_reading_a_frame():
    import pythoncrt_amd as pc

    def never():
        raise AssertionError("a frame was read")
        yield

    for kw, word in ((dict(in_pix_fmt="p010le"), "one end"), (dict(out_pix_fmt="yuv420p10le", in_pix_fmt="nv12"), "one end"),
                     (dict(in_pix_fmt="p010le", out_pix_fmt="p010le", in_size=(36, 160)), "in_size"),
                     (dict(in_pix_fmt="yuv420p10le", out_pix_fmt="p010le", resize_on="host"), "host")):
        with pytest.raises(ValueError) as e:
            pc.process_frames(never(), lambda a: None, 320, 72, 30.0, 1, **kw)
        assert word in str(e.value), (kw, str(e.value))
    fb = model.sizes(72, 320)[2]
    with pytest.raises(ValueError) as e:                                                       # an 8-bit 4:2:0 frame where a 10-bit one is due
        pc.process_frames(iter([np.zeros(fb // 2, dtype=np.uint8)]), lambda a: None, 320, 72, 30.0, 1, in_pix_fmt="p010le", out_pix_fmt="p010le")
    assert str(fb) in str(e.value) and str(fb // 2) in str(e.value)


# ---- CLI ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("io", ["staged", "mapped"])
def test_cli_p010le_in_yuv420p10le_out(tmp_path, io):
    """--in-pix-fmt p010le --out-pix-fmt yuv420p10le over a 3-frame 64 x 96 file (batch 2: a full batch and a short one), --io staged and
    --io mapped: the output file equals what process_frames writes for the same frames, flags and seed, byte for byte."""
    import pythoncrt_amd as pc
    from pythoncrt_amd import cli
    n, h, w = 3, 64, 96
    fb = model.sizes(h, w)[2]
    src = model.to_bytes(np.random.default_rng(45).integers(0, 1024, (n, fb // 2)).astype(np.uint16) << 6).reshape(n, fb)
    (tmp_path / "in.p010").write_bytes(src.tobytes())
    flags = ["--width", str(w), "--height", str(h), "--fps", "30", "--batch", "2", "--noise-seed", "17", "--persistence", "0.3", "--io", io,
             "--in-pix-fmt", "p010le", "--out-pix-fmt", "yuv420p10le", "--out-matrix", "bt709"]
    assert cli.main(flags + ["--input", str(tmp_path / "in.p010"), "--output", str(tmp_path / "out.yuv"), "--staging-report"]) == 0
    got = np.frombuffer((tmp_path / "out.yuv").read_bytes(), dtype=np.uint8)
    assert got.size == n * fb
    want = []
    with open(tmp_path / "in.p010", "rb") as f:
        wrote = pc.process_frames(pc.iter_yuv420(f, w, h, bits=10), lambda a: want.append(np.array(a)), w, h, 30.0, n, noise_seed=17, batch=2,
                                  persistence=0.3, in_pix_fmt="p010le", out_pix_fmt="yuv420p10le", out_matrix="bt709")
    assert wrote == n
    for i in range(n):
        assert np.array_equal(got.reshape(n, fb)[i], want[i]), (io, i, int((got.reshape(n, fb)[i] != want[i]).sum()))
    # ... and the frames are the model's: the first batch of two, then the third frame on the state the first batch left
    from pythoncrt_amd.pipeline import RenderSettings
    rs = RenderSettings(persistence=0.3)
    assert np.array_equal(got.reshape(n, fb), _expected_render(src, (h, w), "p010le", "yuv420p10le", rs, 17, 2, matrix="bt709"))
    with pytest.raises(SystemExit) as e:                                                       # one end only
        cli.main(["--width", str(w), "--height", str(h), "--input", str(tmp_path / "in.p010"), "--output", str(tmp_path / "bad.rgb"), "--io", io,
                  "--in-pix-fmt", "p010le"])
    assert e.value.code not in (0, None) and "one end" in str(e.value) and not (tmp_path / "bad.rgb").exists()
