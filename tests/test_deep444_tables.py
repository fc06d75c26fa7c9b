"""The 10-bit 4:4:4 pair without a GPU: tables.rgb_scale10 and the yuv444p10le tables against the literals of tests/deep444_model.py, the
facts the arithmetic rests on, the integer models against their float64 restatements, the layout helpers, the C-ABI of include/crtfx_444.h
bound symbol for symbol and failing cleanly without a device, the eight kernel builds' registers, and the refusals of process_frames and
the CLI that need no device."""
import ctypes
import io
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pythoncrt_amd import _lib, tables  # noqa: E402
from tests import deep444_model as model  # noqa: E402

N_RANDOM = 2_000_000
K, K2 = 65344, 65729


# ---- tables ----

def test_rgb_scale10_equals_the_literals():
    assert (model.K_IN, model.K_OUT) == (K, K2) == (int(np.floor(1020 / 1023 * 65536 + 0.5)), int(np.floor(1023 / 1020 * 65536 + 0.5)))
    assert tables.rgb_matrix10("bt601", "pc")[0][0] == tables.rgb_matrix10("bt709", "pc")[0][0] == K          # the Y entry
    assert tables.yuv_matrix10("bt601", "pc")[0][:3].sum() == tables.yuv_matrix10("bt709", "pc")[0][:3].sum() == K2      # the Y-row sum
    for order in ("gbr", "rgb"):
        pair = tables.rgb_scale10(order)
        assert len(pair) == 2
        for (m, off), lit in zip(pair, (model.SCALE_IN[order], model.SCALE_OUT[order])):
            assert m.dtype == off.dtype == np.int32 and m.shape == (9,) and off.shape == (3,) and m.flags["C_CONTIGUOUS"] and off.flags["C_CONTIGUOUS"]
            assert m.reshape(3, 3).tolist() == [list(r) for r in lit] and off.tolist() == [0, 0, 0]
            assert (np.count_nonzero(m.reshape(3, 3), axis=0) == 1).all() and (np.count_nonzero(m.reshape(3, 3), axis=1) == 1).all()
    assert np.array_equal(tables.rgb_scale10()[0][0], tables.rgb_scale10("rgb")[0][0])
    src, egr = tables.rgb_scale10("gbr")
    # planes G, B, R: R reads plane 2, G plane 0, B plane 1; plane 0 is written from G, plane 1 from B, plane 2 from R
    assert src[0].reshape(3, 3).argmax(axis=1).tolist() == [2, 0, 1] and egr[0].reshape(3, 3).argmax(axis=1).tolist() == [1, 2, 0]
    for bad in ("bgr", "", "RGB", None):
        with pytest.raises(ValueError):
            tables.rgb_scale10(bad)


@pytest.mark.parametrize("matrix,rng", model.CASES)
def test_yuv_tables_equal_the_literals(matrix, rng):
    for fn, lit in ((tables.rgb_matrix10, model.RGB_MATRICES), (tables.yuv_matrix10, model.YUV_MATRICES)):
        m, off = fn(matrix, rng)
        assert m.reshape(3, 3).tolist() == [list(r) for r in lit[(matrix, rng)]] and tuple(off.tolist()) == model.OFFSETS[rng]
    ms, offs = model.source_table("yuv444p10le", matrix, rng)
    me, offe = model.egress_table("yuv444p10le", matrix, rng)
    assert np.array_equal(ms.reshape(9), tables.rgb_matrix10(matrix, rng)[0]) and np.array_equal(me.reshape(9), tables.yuv_matrix10(matrix, rng)[0])
    assert offs.tolist() == offe.tolist() == list(model.OFFSETS[rng])


def test_the_rgb_formats_ignore_matrix_and_range():
    for fmt in ("gbrp10le", "x2rgb10le"):
        a = model.source_table(fmt)
        for matrix, rng in model.CASES:
            b = model.source_table(fmt, matrix, rng)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- the facts of the full-range RGB scale ----

def _src(v, k=K):
    return np.clip((k * v + (1 << 15)) >> 16, 0, 1020)


def _egr(q, k=K2):
    return np.clip((k * q + (1 << 15)) >> 16, 0, 1023)


def test_rgb_source_scale():
    v = np.arange(1024, dtype=np.int64)
    q = _src(v)
    assert q[0] == 0 and q[1023] == 1020 and (np.diff(q) >= 0).all() and set(q.tolist()) == set(range(1021))
    assert np.abs(q - v * 1020 / 1023).max() <= 0.5015
    for fmt in ("gbrp10le", "x2rgb10le"):                       # the model's tables do that in every channel
        m, off = model.source_table(fmt)
        got = model.quarter_codes(np.stack([v, v, v]), m, off)
        assert np.array_equal(got, np.stack([q, q, q], axis=-1))
    assert (3 * K * 1023 + (1 << 15)) < 2 ** 31


def test_rgb_egress_scale():
    q = np.arange(1021, dtype=np.int64)
    t = _egr(q)
    assert t[0] == 0 and t[1020] == 1023 and (np.diff(t) > 0).all()
    assert K2 * 1020 + (1 << 15) == 67_076_348                  # the accumulator's peak
    for fmt in ("gbrp10le", "x2rgb10le"):
        m, off = model.egress_table(fmt)
        acc = model.accumulators(np.stack([q, q, q], axis=-1), m, off)
        assert acc.min() == 1 << 15 and acc.max() == 67_076_348
        assert np.array_equal(model.convert_codes(np.stack([q, q, q], axis=-1), m, off), np.stack([t, t, t]))


def test_rgb_round_trips():
    """q -> v -> q is exact for 1018 of the 1021 codes: 510 * 1023 / 1020 = 511.5 is a true tie, 510, 849 and 850 return one higher.
    v -> q -> v moves 6 of the 1024 codes by one.  Among the eight neighbouring pairs (K +- 1, K' +- 1) three return 1019 codes — (K, K' - 1),
    (K - 1, K' + 1), (K + 1, K' - 1) — and none more; the constants stay the issue's, which are the full-range tables' own (above)."""
    q = np.arange(1021, dtype=np.int64)
    back = _src(_egr(q))
    assert q[back != q].tolist() == [510, 849, 850] and (back - q)[back != q].tolist() == [1, 1, 1]
    assert 510 * 1023 % 1020 * 2 == 1020                         # the tie
    v = np.arange(1024, dtype=np.int64)
    there = _egr(_src(v))
    assert v[there != v].tolist() == [170, 511, 512, 851, 852, 853] and (np.abs(there - v)[there != v] == 1).all()
    exact = {(dk, dk2): int((_src(_egr(q, K2 + dk2), K + dk) == q).sum()) for dk in (-1, 0, 1) for dk2 in (-1, 0, 1)}
    assert exact[(0, 0)] == 1018 and max(exact.values()) == 1019
    assert sorted(k for k, n in exact.items() if n == 1019) == [(-1, 1), (0, -1), (1, -1)]


# ---- yuv444p10le ----

def test_yuv_egress_accumulators_stay_in_range():
    lows, highs = [], []
    for matrix, rng in model.CASES:
        m, off = model.egress_table("yuv444p10le", matrix, rng)
        for j in range(3):
            konst = (int(off[j]) << 16) + (1 << 15)
            lows.append(konst + int(m[j][m[j] < 0].sum()) * 1020)
            highs.append(konst + int(m[j][m[j] > 0].sum()) * 1020)
        ms = model.source_table("yuv444p10le", matrix, rng)[0]
        assert (np.abs(ms).sum(axis=1) * 1023 + (1 << 15) < 2 ** 31).all()
    assert min(lows) == 32_768 and max(lows) == 4_227_520 and max(highs) == 67_108_480 and max(highs) < 2 ** 31


@pytest.fixture(scope="module")
def colours():
    return np.random.default_rng(0).integers(0, 1021, (N_RANDOM, 3))


@pytest.mark.parametrize("matrix,rng", model.CASES)
def test_yuv_round_trip_and_float_restatements(colours, matrix, rng):
    """2 000 000 random colours of the cube, q -> YUV -> q: within 2 quarter codes at limited range, within 1 at full range.  More than one
    code off at limited range: 0.12 % (bt601) and 0.26 % (bt709) of the channel values, 0.35 % and 0.78 % of the colours.  The integer egress is
    floor(x + 0.5) of the float64 product with the same integer matrix on every sample; the integer source is the float64 one with the
    unrounded matrix except within 3 * 0.5 / 65536 * 1023 = 0.0235 of a half-integer, and there one code apart."""
    me, offe = model.egress_table("yuv444p10le", matrix, rng)
    t = model.convert_codes(colours, me, offe)
    assert int((t != model.convert_codes_float(colours, me, offe)).sum()) == 0
    back = model.quarter_codes(t, *model.source_table("yuv444p10le", matrix, rng))
    err = np.abs(back - colours)
    if rng == "tv":
        assert err.max() == 2
        per_value, per_colour = float((err > 1).mean()), float((err.max(axis=1) > 1).mean())
        want_v, want_c = {"bt601": (0.0012, 0.0035), "bt709": (0.0026, 0.0078)}[matrix]
        assert abs(per_value - want_v) < 0.0001 and abs(per_colour - want_c) < 0.0003, (per_value, per_colour)
    else:
        assert err.max() == 1
    flt, raw = model.quarter_codes_float(t, "yuv444p10le", matrix, rng)
    diff = back - flt
    dist = np.abs(raw - np.floor(raw) - 0.5)
    assert np.abs(diff).max() <= 1 and (diff != 0).any() and (dist[diff != 0] <= 3 * 0.5 / 65536 * 1023).all()


def test_rgb_models_against_the_float_restatements():
    P = np.random.default_rng(5).integers(0, 1024, (3, 200_000))
    q = np.random.default_rng(6).integers(0, 1021, (200_000, 3))
    for fmt in ("gbrp10le", "x2rgb10le"):
        got = model.quarter_codes(P, *model.source_table(fmt))
        flt, raw = model.quarter_codes_float(P, fmt)
        diff = got - flt
        dist = np.abs(raw - np.floor(raw) - 0.5)
        assert np.abs(diff).max() <= 1 and (dist[diff != 0] <= 0.5 / 65536 * 1023).all()
        m, off = model.egress_table(fmt)
        assert int((model.convert_codes(q, m, off) != model.convert_codes_float(q, m, off)).sum()) == 0


def test_every_quarter_code_is_a_half():
    q = np.arange(1021, dtype=np.int64)
    h = model.to_half(q)
    assert h.dtype == np.float16 and np.array_equal(h.astype(np.float64) * 4.0, q.astype(np.float64))
    assert np.array_equal((q / 4.0).astype(np.float32).astype(np.float16), h)             # through float32, as the kernels go
    assert np.array_equal(model.quantise(h), q) and len(set(h.view(np.uint16).tolist())) == 1021
    f = np.array([np.nan, -np.nan, -0.0, 0.0, -1.0, -np.inf, np.inf, 255.0, 300.0, 0.125, 0.375, 0.625], dtype=np.float16)
    assert model.quantise(f).tolist() == [0, 0, 0, 0, 0, 0, 1020, 1020, 1020, 0, 2, 2]


# ---- layout ----

@pytest.mark.parametrize("h,w", [(1, 1), (2, 3), (3, 5), (16, 64), (37, 131)])
def test_frame_bytes_layouts_and_helpers(h, w):
    import torch
    from pythoncrt_amd import deep444
    assert [deep444.frame_bytes(h, w, f) for f in model.FORMATS] == [model.sizes(h, w, f) for f in model.FORMATS] == [6 * h * w, 6 * h * w, 4 * h * w]
    p = model.images(h, w)[0]
    assert p.shape == (6 * h * w,) and p.dtype == np.uint8
    P = model.samples(p, h, w, "yuv444p10le")
    wd = p.view("<u2").astype(np.int64)
    assert wd.max() <= 1023 and np.array_equal(P, wd.reshape(3, h, w)) and np.array_equal(model.samples(p, h, w, "gbrp10le"), P)
    x = model.relayout(p, h, w, "x2rgb10le")
    xw = x.view("<u4").astype(np.int64).reshape(h, w)
    assert x.shape == (4 * h * w,) and np.array_equal(xw, (P[0] << 20) | (P[1] << 10) | P[2]) and not (xw >> 30).any()
    assert np.array_equal(model.relayout(p, h, w, "gbrp10le"), p)
    # the bits outside a sample are ignored when read
    assert np.array_equal(model.samples((wd | 0xFC00).astype("<u2").view(np.uint8), h, w, "yuv444p10le"), P)
    assert np.array_equal(model.samples((xw | (3 << 30)).astype("<u4").reshape(-1).view(np.uint8), h, w, "x2rgb10le"), P)
    # the same samples under one table give the same halves from both layouts; gbrp10le holds G, B, R
    a = model.unpack(p, h, w, "gbrp10le")
    b = model.unpack(model.pack_samples(P[[2, 0, 1]], "x2rgb10le"), h, w, "x2rgb10le")
    assert a.shape == (h, w, 3) and a.dtype == np.float16 and np.array_equal(a.view(np.uint16), b.view(np.uint16))
    assert np.array_equal(model.quantise(a)[..., 1], model.quarter_codes(P, *model.source_table("x2rgb10le"))[..., 0])      # G is plane 0
    # pack is the inverse layout: planes G, B, R / fields R, G, B of the same halves
    g = model.samples(model.pack(a, "gbrp10le"), h, w, "gbrp10le")
    r = model.samples(model.pack(a, "x2rgb10le"), h, w, "x2rgb10le")
    assert np.array_equal(g, r[[1, 2, 0]])
    # the product's helpers: word views, numpy and torch, one frame and a batch
    for fmt in ("yuv444p10le", "gbrp10le"):
        planes = deep444.split_planes(p, (h, w), fmt)
        assert len(planes) == 3 and all(q.dtype == np.uint16 and q.shape == (h, w) and np.shares_memory(q, p) for q in planes)
        assert np.array_equal(np.stack(planes), P)
    (words,) = deep444.split_planes(x, (h, w), "x2rgb10le")
    assert words.dtype == np.uint32 and words.shape == (h, w) and np.array_equal(words, xw)
    ty = deep444.split_planes(torch.from_numpy(np.stack([p, p])), (h, w), "yuv444p10le")
    assert ty[0].dtype == torch.int16 and tuple(ty[2].shape) == (2, h, w) and np.array_equal(ty[2][1].numpy().view(np.uint16), P[2])
    (tw,) = deep444.split_planes(torch.from_numpy(np.stack([x, x])), (h, w), "x2rgb10le")
    assert tw.dtype == torch.int32 and tuple(tw.shape) == (2, h, w) and np.array_equal(tw[1].numpy().view(np.uint32), xw)
    with pytest.raises(ValueError):
        deep444.split_planes(p[:-2], (h, w), "yuv444p10le")
    for bad in ("yuv444p", "p010le", "gbrp"):
        with pytest.raises(ValueError):
            deep444.split_planes(p, (h, w), bad)
        with pytest.raises(ValueError):
            deep444.frame_bytes(h, w, bad)


def test_images_hold_what_they_are_to_hold():
    h, w = 270, 480
    rand, binary, pal = (model.samples(p, h, w, "yuv444p10le") for p in model.images(h, w))
    assert rand.max() == 1023 and len(set(rand.reshape(-1).tolist())) == 1024 and set(binary.reshape(-1).tolist()) == {0, 1023}
    assert set(map(tuple, pal.reshape(3, -1).T.tolist())) == set(model.PALETTE) and len(model.PALETTE) == 13 + 1024 + 8
    m = np.array(model.RGB_MATRICES[("bt601", "tv")], dtype=np.int64)

    def before_clamp(yy, uu, vv):
        return (m @ np.array([yy - 64, uu - 512, vv - 512], dtype=np.int64) + (1 << 15)) >> 16
    assert before_clamp(940, 512, 960)[0] > 1020 and before_clamp(64, 64, 64)[0] < 0 and before_clamp(64, 64, 64)[2] < 0 and before_clamp(64, 960, 960)[1] < 0
    for col in ((940, 512, 960), (64, 64, 64), (64, 960, 960)):
        assert col in model.PALETTE


def test_iter_deep444_reads_whole_frames():
    import pythoncrt_amd as pc
    h, w = 5, 7

    class Dribble(io.BytesIO):                                  # a pipe may return less than asked for
        def read(self, n=-1):
            return super().read(min(n, 11) if n and n > 0 else n)
    for fmt in model.FORMATS:
        fb = model.sizes(h, w, fmt)
        data = np.random.default_rng(4).integers(0, 256, 3 * fb + fb // 2, dtype=np.uint8)
        for stream in (io.BytesIO(data.tobytes()), Dribble(data.tobytes())):
            frames = list(pc.iter_deep444(stream, w, h, fmt))
            assert len(frames) == 3 and all(f.shape == (fb,) and f.dtype == np.uint8 for f in frames)
            assert np.array_equal(np.concatenate(frames), data[:3 * fb])
    with pytest.raises(ValueError):
        next(pc.iter_deep444(io.BytesIO(b""), w, h, "yuv444p"))


# ---- C ABI ----

FAMILIES = ("unpack444", "egress444")


def test_header_prototypes_are_the_bound_symbols():
    """include/crtfx_444.h declares exactly _lib.DEEP444_SYMBOLS (argument counts included): two families of seven that mirror
    crtfx_unpack10_* signature for signature; the table shares no name with the other families; both new files are sources of the build;
    the built library exports every symbol."""
    hdr = open(os.path.join(ROOT, "include", "crtfx_444.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(crtfx_(?:unpack444|egress444)_\w+)\s*\(([^)]*)\)\s*;", hdr)}
    assert set(protos) == set(_lib.DEEP444_SYMBOLS) and len(protos) == 14, set(protos) ^ set(_lib.DEEP444_SYMBOLS)
    assert {n.split("_", 2)[2] for n in protos} == {"create", "destroy", "last_error", "frame_bytes", "run", "set_option", "last_plan"}
    others = set(_lib.SYMBOLS) | set(_lib.INGEST_SYMBOLS) | set(_lib.EGRESS_SYMBOLS) | set(_lib.UNPACK_SYMBOLS) | set(_lib.DEEP_SYMBOLS) | set(_lib.YUV422_SYMBOLS)
    assert not set(_lib.DEEP444_SYMBOLS) & others
    for name, args in protos.items():
        n_args = 0 if args.strip() in ("", "void") else len(args.split(","))
        assert n_args == len(_lib.DEEP444_SYMBOLS[name][1]), name
        assert _lib.DEEP444_SYMBOLS[name] == _lib.DEEP_SYMBOLS[name.replace("unpack444", "unpack10").replace("egress444", "unpack10")], name
    assert re.search(r"CRTFX_444_PLANAR\s*=\s*0\s*,\s*CRTFX_444_X2RGB10LE\s*=\s*1", hdr)
    assert re.search(r"CRTFX_UNPACK444_OPT_FORCE_GENERAL\s*=\s*1", hdr) and re.search(r"CRTFX_EGRESS444_OPT_FORCE_GENERAL\s*=\s*1", hdr)
    assert (_lib.DEEP444_PLANAR, _lib.DEEP444_X2RGB10LE, _lib.UNPACK444_OPT_FORCE_GENERAL, _lib.EGRESS444_OPT_FORCE_GENERAL) == (0, 1, 1, 1)
    assert all(os.path.basename(f) in {os.path.basename(s) for s in _lib.SOURCES} for f in ("crtfx_444.hip", "crtfx_444.h"))
    lib = _lib.load()
    for name in _lib.DEEP444_SYMBOLS:
        assert getattr(lib, name).argtypes == _lib.DEEP444_SYMBOLS[name][1]
    import pythoncrt_amd as pc
    from pythoncrt_amd import deep444
    assert pc.UnpackDeep444.__name__ in pc.__all__ and pc.EgressDeep444.__name__ in pc.__all__ and "iter_deep444" in pc.__all__
    assert deep444.FORMATS == {"yuv444p10le": 0, "gbrp10le": 0, "x2rgb10le": 1}


def _table(fam, order=None):
    if order:
        return tables.rgb_scale10(order)[fam == "egress444"]
    return (tables.rgb_matrix10 if fam == "unpack444" else tables.yuv_matrix10)("bt601", "tv")


def _create(lib, fam, h=12, w=20, pix_fmt=_lib.PIX_F16, layout=_lib.DEEP444_PLANAR, device=0, m=None, off=None, null=False, null_off=False, order=None):
    tm, toff = _table(fam, order)
    m = tm if m is None else np.ascontiguousarray(m, dtype=np.int32)
    off = toff if off is None else np.ascontiguousarray(off, dtype=np.int32)
    plan = ctypes.c_void_p(1)
    rc = getattr(lib, f"crtfx_{fam}_create")(device, h, w, pix_fmt, layout, None if null else tables.ptr(m), None if null_off else tables.ptr(off),
                                             ctypes.byref(plan))
    return rc, plan, (getattr(lib, f"crtfx_{fam}_last_error")(None) or b"").decode()


@pytest.mark.parametrize("fam", FAMILIES)
def test_create_refuses_bad_arguments_before_it_touches_a_device(fam):
    """The argument checks come first, so they hold on any machine: uint8 frames are UNSUPPORTED and the message names half; a size < 1 or
    > 32767, an unknown layout or pixel format, a null table, an offset outside 0..1023 and a matrix whose accumulator could leave its range
    are INVALID; each leaves *out_plan NULL and a message.  The largest matrix still admitted, and the one just over it."""
    lib = _lib.load()
    good = _table(fam)[0]
    too_big, too_negative, fits = good.copy(), good.copy(), good.copy()
    if fam == "unpack444":
        too_big[8] = 1 << 21                                  # B row: 1023 * (76309 + 132201 + 2^21) + 2^15 passes 2^31
        too_negative[4] = -(1 << 21)                          # G row: the rule sums magnitudes
        fits[6:9] = (2099169, 0, 0)                           # 1023 * 2099169 + 2^15 = 2^31 - 993: admitted (2099170 is not)
        over = fits.copy()
        over[6] += 1
    else:
        too_big[6] = 1 << 21                                  # V row: 1020 * 2^21 passes 2^31
        too_negative[4] = -40000                              # U row: (512 << 16) + 2^15 - 1020 * (9714 + 40000) < 0
        fits[3:6] = (-32928, 0, 2072447)                      # U row: K = 33587200; K - 32928 * 1020 = 640 >= 0, K + 2072447 * 1020 = 2^31 - 508
        over = fits.copy()
        over[5] += 1                                          # ... 2^31 + 512
        under = fits.copy()
        under[3] -= 1                                         # ... 640 - 1020 < 0
    assert (1023 * 2099169 + (1 << 15), 33587200 + 2072447 * 1020, 33587200 - 32928 * 1020) == (2 ** 31 - 993, 2 ** 31 - 508, 640)
    cases = [(dict(m=over), _lib.E_INVALID, "accumulator"), (dict(pix_fmt=_lib.PIX_U8), _lib.E_UNSUPPORTED, "half"), (dict(h=0), _lib.E_INVALID, "size"),
             (dict(w=0), _lib.E_INVALID, "size"), (dict(w=40000), _lib.E_INVALID, "size"), (dict(h=32768), _lib.E_INVALID, "size"),
             (dict(null=True), _lib.E_INVALID, "null"), (dict(null_off=True), _lib.E_INVALID, "null"),
             (dict(pix_fmt=7), _lib.E_INVALID, "pixel format"), (dict(layout=2), _lib.E_INVALID, "layout"), (dict(layout=-1), _lib.E_INVALID, "layout"),
             (dict(off=(64, 1024, 512)), _lib.E_INVALID, "offset"), (dict(off=(-1, 512, 512)), _lib.E_INVALID, "offset"),
             (dict(m=too_big), _lib.E_INVALID, "accumulator"), (dict(m=too_negative), _lib.E_INVALID, "accumulator")]
    if fam == "egress444":
        cases.append((dict(m=under), _lib.E_INVALID, "accumulator"))
    for kw, code, word in cases:
        rc, plan, msg = _create(lib, fam, **kw)
        assert rc == code and not plan.value and word in msg, (kw, rc, plan.value, msg)
    rc = getattr(lib, f"crtfx_{fam}_create")(0, 8, 8, _lib.PIX_F16, 0, tables.ptr(good), tables.ptr(_table(fam)[1]), None)
    assert rc == _lib.E_INVALID and b"out_plan" in getattr(lib, f"crtfx_{fam}_last_error")(None)
    admitted = [dict(m=fits), dict(off=(1023, 0, 1023)) if fam == "unpack444" else dict(off=(64, 512, 512)), dict(h=32767, w=32767),
                dict(order="gbr"), dict(order="rgb", layout=_lib.DEEP444_X2RGB10LE)]
    for kw in admitted:
        rc, plan, msg = _create(lib, fam, **kw)
        assert rc in (_lib.OK, _lib.E_HIP), (kw, rc, msg)         # no device here: E_HIP; with one: a plan
        if rc == _lib.OK:
            assert getattr(lib, f"crtfx_{fam}_destroy")(plan) == _lib.OK
    f = lambda name: getattr(lib, f"crtfx_{fam}_{name}")          # noqa: E731
    assert f("destroy")(None) == _lib.OK and f("set_option")(None, 1, 1) == _lib.E_INVALID
    assert f("run")(None, None, 0, None, 0, 1, None) == _lib.E_INVALID and f("frame_bytes")(None) == 0
    assert f("last_plan")(None, ctypes.create_string_buffer(8), 8) == _lib.E_INVALID
    assert f("last_error")(None) is not None


@pytest.mark.parametrize("fam", FAMILIES)
def test_create_without_a_gpu_fails_cleanly(fam):
    import torch
    lib = _lib.load()
    if torch.cuda.is_available():
        rc, plan, msg = _create(lib, fam, device=4096)          # no such device on any box
        assert rc == _lib.E_HIP and not plan.value and "4096" in msg
        return
    rc, plan, msg = _create(lib, fam)
    assert rc == _lib.E_HIP and not plan.value and msg, (rc, msg)


def test_the_eight_kernel_builds_and_their_registers():
    """Exactly eight kernel builds (two directions x two layouts x two paths) under crtfx_444_impl:: in the library's code objects
    (tools/kernel_resources.py): no spills, no scratch memory, no LDS, at most 128 VGPRs + AGPRs.  include/crtfx_444.h states the counts
    the build shows."""
    import kernel_resources
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    res = kernel_resources.resources(_lib.LIB_PATH)
    found = {n: v for n, v in res.items() if n.startswith("crtfx_444_impl::")}
    layouts, paths = {"planar": 0, "x2rgb10le": 1}, {"general": 0, "vec": 1}
    names = {(d, l, p): f"crtfx_444_impl::k_{d}10_444<{layouts[l]}, {paths[p]}>" for d in ("unpack", "egress") for l in layouts for p in paths}
    assert set(found) == set(names.values()) and len(found) == 8, sorted(found)
    for name, v in found.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["group_segment_fixed_size"] == 0 and v["vgpr_count"] + v["agpr_count"] <= 128 and v["agpr_count"] == 0, (name, v)
    hdr = open(os.path.join(ROOT, "include", "crtfx_444.h")).read()
    stated = {}
    for d in ("unpack", "egress"):
        seg = re.search(rf"k_{d}10_444 ((?:<\w+,\w+> \d+,?\s*(?:\*\s*)?)+)VGPRs", hdr)
        assert seg, f"the header's register line of k_{d}10_444"
        for l, p, n in re.findall(r"<(\w+),(\w+)> (\d+)", seg.group(1)):
            stated[(d, l, p)] = int(n)
    assert set(stated) == set(names)
    for key, name in names.items():
        assert stated[key] == found[name]["vgpr_count"], (key, stated[key], found[name]["vgpr_count"])


# ---- refusals that need no device ----

def test_process_frames_refuses_before_it_touches_a_device():
    """A new format against an 8-bit name, an in_size other than the output size and resize_on="host": ValueError, each message names its
    reason, no frame is read and nothing is written.  yuv444p stays unknown, and the unknown-name messages keep their leading text."""
    import pythoncrt_amd as pc

    def never():
        raise AssertionError("a frame was read")
        yield

    def call(**kw):
        return pc.process_frames(never(), lambda a: (_ for _ in ()).throw(AssertionError("written")), 64, 36, 30.0, 1, **kw)
    cases = []
    for fmt in model.FORMATS:
        cases += [(dict(in_pix_fmt=fmt), "one end"), (dict(out_pix_fmt=fmt), "one end"), (dict(in_pix_fmt=fmt, out_pix_fmt="nv12"), "one end"),
                  (dict(in_pix_fmt="yuyv422", out_pix_fmt=fmt), "one end"),
                  (dict(in_pix_fmt=fmt, out_pix_fmt="p010le", in_size=(18, 32)), "in_size"),
                  (dict(in_pix_fmt=fmt, out_pix_fmt=fmt, resize_on="host"), "host"),
                  (dict(in_pix_fmt="p010le", out_pix_fmt=fmt, resize_on="host"), "host"),
                  (dict(in_pix_fmt="yuv444p", out_pix_fmt=fmt), "in_pix_fmt must be 'rgb24', 'yuv420p' or 'nv12'"),
                  (dict(in_pix_fmt=fmt, out_pix_fmt="yuv444p12le"), "out_pix_fmt must be 'rgb24', 'yuv420p' or 'nv12'")]
    for kw, word in cases:
        with pytest.raises(ValueError) as e:
            call(**kw)
        assert word in str(e.value), (kw, str(e.value))
    for side in ("in_pix_fmt", "out_pix_fmt"):
        with pytest.raises(ValueError) as e:
            call(**{side: "yuv444p"})
        assert all(f"'{f}'" in str(e.value) for f in model.FORMATS)      # the new names are appended to the message


def test_cli_refuses_before_it_touches_a_device(monkeypatch, tmp_path):
    """One end only: SystemExit that names both flags.  The sharded CLI refuses the new formats as it refuses every non-rgb24 one.  The parser
    takes the three names and still rejects yuv444p."""
    from pythoncrt_amd import cli
    src = tmp_path / "in.raw"
    src.write_bytes(bytes(8 * 8 * 6))
    base = ["--input", str(src), "--output", str(tmp_path / "out.raw"), "--width", "8", "--height", "8"]
    for fmt in model.FORMATS:
        for extra in (["--in-pix-fmt", fmt], ["--out-pix-fmt", fmt], ["--in-pix-fmt", fmt, "--out-pix-fmt", "nv12"], ["--in-pix-fmt", "uyvy422", "--out-pix-fmt", fmt]):
            with pytest.raises(SystemExit) as e:
                cli.main(base + extra)
            assert e.value.code not in (0, None) and "one end" in str(e.value) and "--in-pix-fmt" in str(e.value) and "--out-pix-fmt" in str(e.value)
            assert not (tmp_path / "out.raw").exists()
    parser = cli.add_input_flags(cli.add_output_flags(cli.build_parser()))
    for a_fmt, b_fmt in (("yuv444p10le", "gbrp10le"), ("x2rgb10le", "p010le"), ("p010le", "x2rgb10le")):
        a = parser.parse_args(["--input", "x", "--in-pix-fmt", a_fmt, "--out-pix-fmt", b_fmt])
        assert (a.in_pix_fmt, a.out_pix_fmt) == (a_fmt, b_fmt)
    for flag in ("--in-pix-fmt", "--out-pix-fmt"):
        with pytest.raises(SystemExit):
            parser.parse_args(["--input", "x", flag, "yuv444p"])
    assert cli.DEEP_PIX_FMTS == ("yuv420p10le", "p010le") and cli.DEEP444_PIX_FMTS == model.FORMATS
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    for fmt in model.FORMATS:
        with pytest.raises(SystemExit) as e:
            cli.main(base + ["--in-pix-fmt", fmt, "--out-pix-fmt", fmt])
        assert fmt in str(e.value) and "sharded" in str(e.value) and not (tmp_path / "out.raw").exists()
