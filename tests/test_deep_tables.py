"""The 10-bit pair without a GPU: tables.rgb_matrix10 / yuv_matrix10 against the eight literal matrices of tests/deep_model.py, the
identities the arithmetic rests on, the integer models against their float64 restatements, the round trip source -> egress, the C-ABI of
include/crtfx_deep.h bound symbol for symbol and failing cleanly without a device, the eight kernel builds' registers, the layout helpers
and the refusals of process_frames and the CLI that need no device."""
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
from tests import deep_model as model  # noqa: E402

N_RANDOM = 1_000_000


# ---- matrices -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("matrix,rng", model.CASES)
def test_matrices_equal_the_literals(matrix, rng):
    for fn, lit, eight in ((tables.rgb_matrix10, model.RGB_MATRICES, tables.rgb_matrix), (tables.yuv_matrix10, model.YUV_MATRICES, tables.yuv_matrix)):
        m, off = fn(matrix, rng)
        assert m.dtype == off.dtype == np.int32 and m.shape == (9,) and off.shape == (3,) and m.flags["C_CONTIGUOUS"] and off.flags["C_CONTIGUOUS"]
        assert m.reshape(3, 3).tolist() == [list(r) for r in lit[(matrix, rng)]]
        assert tuple(off.tolist()) == model.OFFSETS[rng]
        m8, off8 = eight(matrix, rng)
        assert off.tolist() == [4 * o for o in off8.tolist()]                 # 10-bit limited range is 4 x the 8-bit one, offsets included
        if rng == "tv":
            assert np.array_equal(m, m8)                                        # ... so the limited-range matrices are the 8-bit ones
        else:
            assert not np.array_equal(m, m8)
    for bad in (("bt2020", "tv"), ("bt601", "full")):
        with pytest.raises(ValueError):
            tables.rgb_matrix10(*bad)
        with pytest.raises(ValueError):
            tables.yuv_matrix10(*bad)


@pytest.mark.parametrize("matrix,rng", model.CASES)
def test_matrices_follow_the_stated_recipes(matrix, rng):
    rgb = np.array(model.RGB_MATRICES[(matrix, rng)], dtype=np.int64)
    assert np.array_equal(rgb, np.floor(model.rgb_float_matrix(matrix, rng) * 65536 + 0.5).astype(np.int64))     # none adjusted
    assert rgb[0, 1] == 0 and rgb[2, 2] == 0                                  # R,U and B,V: exactly 0
    assert rgb[0, 0] == rgb[1, 0] == rgb[2, 0]                                # the three Y entries are one number
    yuv = np.array(model.YUV_MATRICES[(matrix, rng)], dtype=np.int64)
    f = np.floor(model.yuv_float_matrix(matrix, rng) * 65536 + 0.5).astype(np.int64)
    assert np.array_equal(yuv[:, [0, 2]], f[:, [0, 2]]) and (np.abs(yuv[:, 1] - f[:, 1]) <= 1).all()              # the G entry carries the adjustment
    sy = (876.0 / 1020.0) if rng == "tv" else (1023.0 / 1020.0)
    assert yuv[0].sum() == int(np.floor(sy * 65536 + 0.5)) and yuv[1].sum() == 0 and yuv[2].sum() == 0


@pytest.mark.parametrize("matrix,rng", model.CASES)
def test_identities(matrix, rng):
    """Every grey gives U = V = 512 and R = G = B; limited 64 <-> 0 and 940 <-> 1020 <-> 255.0 both ways; full 1023 -> 1020 -> 1023."""
    off = model.OFFSETS[rng]
    g = np.arange(1021, dtype=np.int64)
    grey = np.repeat(g[None, :, None], 3, axis=2)                              # 1 x 1021 x 3: every quarter-code grey
    y, u, v = model.convert_codes(np.repeat(np.repeat(grey, 2, axis=0), 2, axis=1), matrix, rng)
    assert (u == 512).all() and (v == 512).all() and (np.diff(y[0]) >= 0).all()
    codes = np.arange(1024, dtype=np.int64)
    q = model.quarter_codes(codes - off[0], np.zeros_like(codes), np.zeros_like(codes), matrix, rng)
    assert np.array_equal(q[:, 0], q[:, 1]) and np.array_equal(q[:, 1], q[:, 2]) and (np.diff(q[:, 0]) >= 0).all()
    white = model.to_half(np.array([1020]))
    assert white.dtype == np.float16 and float(white[0]) == 255.0
    if rng == "tv":
        assert q[64, 0] == 0 and q[940, 0] == 1020 and q[:64].max() == 0 and q[940:].min() == 1020
        assert y[0, 0] == 64 and y[0, 2 * 1020] == 940
    else:
        assert q[0, 0] == 0 and q[1023, 0] == 1020
        assert y[0, 0] == 0 and y[0, 2 * 1020] == 1023
    # full range with a grey pixel: Y = q is NOT an identity (1023/1020), but q -> Y is injective and monotone at both ranges' ends
    assert len(set(y[0, ::2].tolist())) == (877 if rng == "tv" else 1021)


@pytest.mark.parametrize("matrix,rng", model.CASES)
def test_accumulators_stay_inside_int32(matrix, rng):
    """The rules crtfx_unpack10_create and crtfx_egress10_create check, on the eight matrices."""
    rgb = np.array(model.RGB_MATRICES[(matrix, rng)], dtype=np.int64)
    assert (np.abs(rgb).sum(axis=1) * 1023 + (1 << 15) < 2 ** 31).all()
    yuv, off = np.array(model.YUV_MATRICES[(matrix, rng)], dtype=np.int64), model.OFFSETS[rng]
    for row, konst, x in ((yuv[0], (off[0] << 16) + (1 << 15), 1020), (yuv[1], (off[1] << 18) + (1 << 17), 4080), (yuv[2], (off[2] << 18) + (1 << 17), 4080)):
        assert konst + row[row < 0].sum() * x >= 0 and konst + row[row > 0].sum() * x < 2 ** 31, (row, konst)


def test_every_quarter_code_is_a_half():
    q = np.arange(1021, dtype=np.int64)
    h = model.to_half(q)
    assert h.dtype == np.float16 and np.array_equal(h.astype(np.float64) * 4.0, q.astype(np.float64))
    assert np.array_equal((q / 4.0).astype(np.float32).astype(np.float16), h)             # through float32, as the kernels go
    assert np.array_equal(model.quantise(h), q)                                            # and the egress quantiser reads each back
    assert len(set(h.view(np.uint16).tolist())) == 1021


def test_the_quantiser_on_the_special_values():
    f = np.array([np.nan, -np.nan, -0.0, 0.0, -1.0, -np.inf, np.inf, 255.0, 300.0, 65504.0, 0.125, 0.375, 0.625, 6e-8, 254.875], dtype=np.float16)
    assert model.quantise(f).tolist() == [0, 0, 0, 0, 0, 0, 1020, 1020, 1020, 1020, 0, 2, 2, 0, 1020]       # ties go to even
    every = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    q = model.quantise(every)
    assert q.min() == 0 and q.max() == 1020 and len(set(q.tolist())) == 1021


# ---- the integer models against the float64 restatements ----------------------------------------------------------------------------------

@pytest.mark.parametrize("matrix,rng", model.CASES)
def test_source_model_against_the_float_restatement(matrix, rng):
    """Random (Y, U, V) triples: the integer quarter code is the float64 one (round-half-up of F . (c, d, e), clamped) except where the
    float value sits within 3 * 0.5 / 65536 * 1023 = 0.0235 of a half-integer — the most the rounding of three coefficients to 2^-16 can move
    the sum for inputs up to 1023 in magnitude — and there it differs by one code.  (On 3 M samples per matrix: 0.07 - 0.14 % differ, the
    largest distance 0.0066.)"""
    yuv = np.random.default_rng(21).integers(0, 1024, (N_RANDOM, 3))
    off = model.OFFSETS[rng]
    c, d, e = yuv[:, 0] - off[0], yuv[:, 1] - off[1], yuv[:, 2] - off[2]
    got = model.quarter_codes(c, d, e, matrix, rng)
    exp, raw = model.quarter_codes_float(c, d, e, matrix, rng)
    diff = got - exp
    assert np.abs(diff).max() <= 1
    bound = 3 * 0.5 / 65536 * 1023
    dist = np.abs(raw - np.floor(raw) - 0.5)
    assert (diff != 0).any() and (dist[diff != 0] <= bound).all(), float(dist[diff != 0].max())


@pytest.mark.parametrize("matrix,rng", model.CASES)
def test_egress_model_against_the_float_restatement(matrix, rng):
    """Random quarter codes: Y, U and V are the float64 ones (round-half-up of F . q + off, chroma from the float mean S / 4) except where
    the float value sits within (0.5 + 0.5 + 1.5) / 65536 * 1020 = 0.039 of a half-integer — two rounded entries and the adjusted G entry —
    and there they differ by one code.  (On 3 M samples per matrix: 0.10 - 0.23 % differ.)"""
    q = np.random.default_rng(22).integers(0, 1021, (2, N_RANDOM // 2, 3))
    ints = model.convert_codes(q, matrix, rng)
    floats, raws = model.convert_codes_float(q, matrix, rng)
    bound = (0.5 + 0.5 + 1.5) / 65536 * 1020
    for name, got, exp, raw in zip("YUV", ints, floats, raws):
        diff = got - exp
        assert np.abs(diff).max() <= 1, name
        dist = np.abs(raw - np.floor(raw) - 0.5)
        assert (dist[diff != 0] <= bound).all(), (name, float(dist[diff != 0].max()))


@pytest.mark.parametrize("matrix,rng", model.CASES)
def test_round_trip_source_to_egress(matrix, rng):
    """Uniform 2 x 2 blocks of random (Y, U, V) whose colour lies inside the RGB cube (no channel clamps): egress(source(yuv)) is yuv at
    limited range — 877 / 897 codes go into 1021 quarter codes — and within 1 code at full range."""
    yuv = np.random.default_rng(23).integers(0, 1024, (N_RANDOM, 3))
    off = model.OFFSETS[rng]
    c, d, e = yuv[:, 0] - off[0], yuv[:, 1] - off[1], yuv[:, 2] - off[2]
    _, raw = model.quarter_codes_float(c, d, e, matrix, rng)
    inside = ((raw >= 0) & (raw <= 1020)).all(axis=1)
    assert inside.sum() > N_RANDOM // 10
    q = model.quarter_codes(c[inside], d[inside], e[inside], matrix, rng)
    img = np.repeat(np.repeat(q[None, :, :], 2, axis=0), 2, axis=1)           # 2 x (2 n) x 3
    y, u, v = model.convert_codes(img, matrix, rng)
    src = yuv[inside]
    err = max(np.abs(y[0, ::2] - src[:, 0]).max(), np.abs(y[1, 1::2] - src[:, 0]).max(), np.abs(u[0] - src[:, 1]).max(), np.abs(v[0] - src[:, 2]).max())
    assert err <= (0 if rng == "tv" else 1), int(err)
    # ... and through the bytes: pack(unpack(frame)) of both layouts gives the frame's samples back
    n = 64
    for layout in model.LAYOUTS:
        frame = model.pack_planes(np.repeat(np.repeat(src[None, :n, 0], 2, axis=0), 2, axis=1), src[None, :n, 1], src[None, :n, 2], layout)
        back = model.pack(model.unpack(frame, 2, 2 * n, layout, matrix, rng), layout, matrix, rng)
        assert np.abs(model.words(back).astype(np.int64) - model.words(frame).astype(np.int64)).max() <= ((0 if rng == "tv" else 1) << (6 if layout == "p010le" else 0))


# ---- layout -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (3, 5), (37, 131), (16, 64)])
def test_frame_bytes_plane_offsets_and_helpers(h, w):
    from pythoncrt_amd import deep
    ch, cw, fb = model.sizes(h, w)
    assert deep.frame_bytes(h, w) == fb == 2 * (h * w + 2 * ch * cw) and (ch, cw) == (-(-h // 2), -(-w // 2))
    p = model.images(h, w)[0]
    assert p.shape == (fb,) and p.dtype == np.uint8
    y, u, v = model.planes(p, h, w, "yuv420p10le")
    wd = model.words(p).astype(np.int64)
    assert wd.max() <= 1023 and np.array_equal(y, wd[:h * w].reshape(h, w))
    assert np.array_equal(u, wd[h * w:h * w + ch * cw].reshape(ch, cw)) and np.array_equal(v, wd[h * w + ch * cw:].reshape(ch, cw))
    q = model.relayout(p, h, w, "p010le")
    qw = model.words(q).astype(np.int64)
    assert q.shape == (fb,) and np.array_equal(qw[:h * w], wd[:h * w] << 6) and not (qw & 63).any()
    assert np.array_equal(qw[h * w::2].reshape(ch, cw), u << 6) and np.array_equal(qw[h * w + 1::2].reshape(ch, cw), v << 6)
    for t in model.planes(q, h, w, "p010le"), model.planes(model.to_bytes(qw | 63), h, w, "p010le"), model.planes(model.to_bytes(wd | 0xFC00), h, w, "yuv420p10le"):
        assert np.array_equal(t[0], y) and np.array_equal(t[1], u) and np.array_equal(t[2], v)     # the bits outside the sample are ignored
    # the product's helpers: 16-bit views, numpy and torch, one frame and a batch
    py, pu, pv = deep.split_planes(p, (h, w), "yuv420p10le")
    qy, quv = deep.split_planes(q, (h, w), "p010le")
    assert py.dtype == np.uint16 and np.shares_memory(py, p) and py.shape == (h, w) and pu.shape == pv.shape == (ch, cw) and quv.shape == (ch, cw, 2)
    assert np.array_equal(py, y) and np.array_equal(pu, u) and np.array_equal(pv, v)
    assert np.array_equal(qy >> 6, y) and np.array_equal(quv[..., 0] >> 6, u) and np.array_equal(quv[..., 1] >> 6, v)
    import torch
    batch = torch.from_numpy(np.stack([p, p]))
    ty, tu, tv = deep.split_planes(batch, (h, w), "yuv420p10le")
    assert ty.dtype == torch.int16 and tuple(ty.shape) == (2, h, w) and tuple(tu.shape) == tuple(tv.shape) == (2, ch, cw)
    assert np.array_equal(ty[1].numpy().view(np.uint16), y) and np.array_equal(tv[0].numpy().view(np.uint16), v)
    with pytest.raises(ValueError):
        deep.split_planes(p[:-2], (h, w), "yuv420p10le")
    with pytest.raises(ValueError):
        deep.split_planes(p, (h, w), "nv12")
    # the same samples give the same halves in both layouts; every pixel reads chroma sample (y >> 1, x >> 1), the odd edge the last one
    a, b = model.unpack(p, h, w, "yuv420p10le"), model.unpack(q, h, w, "p010le")
    assert a.shape == (h, w, 3) and a.dtype == np.float16 and np.array_equal(a.view(np.uint16), b.view(np.uint16))
    c, d, e = model.terms(p, h, w, "yuv420p10le", "tv")
    for yy, xx in ((0, 0), (h - 1, 0), (0, w - 1), (h // 2, w // 2), (h - 1, w - 1)):
        assert d[yy, xx] == u[yy >> 1, xx >> 1] - 512 and e[yy, xx] == v[yy >> 1, xx >> 1] - 512 and c[yy, xx] == y[yy, xx] - 64


def test_images_hold_what_they_are_to_hold():
    h, w = 270, 480
    rand, binary, pal = model.images(h, w)
    assert model.words(rand).max() <= 1023 and len(set(model.words(rand).tolist())) == 1024
    assert set(model.words(binary).tolist()) == {0, 1023}
    y, u, v = model.planes(pal, h, w, "yuv420p10le")
    seen = set(zip(y[::2, ::2].reshape(-1).tolist(), u.reshape(-1).tolist(), v.reshape(-1).tolist()))
    assert seen == set(model.PALETTE) and len(model.PALETTE) == 13 + 1024 + 8
    m = np.array(model.RGB_MATRICES[("bt601", "tv")], dtype=np.int64)

    def before_clamp(yy, uu, vv):
        return (m @ np.array([yy - 64, uu - 512, vv - 512], dtype=np.int64) + (1 << 15)) >> 16
    assert before_clamp(940, 512, 960)[0] > 1020 and before_clamp(64, 64, 64)[0] < 0 and before_clamp(64, 64, 64)[2] < 0 and before_clamp(64, 960, 960)[1] < 0
    for col in ((940, 512, 960), (64, 64, 64), (64, 960, 960)):
        assert col in model.PALETTE


def test_iter_yuv420_reads_ten_bit_frames():
    import pythoncrt_amd as pc
    h, w = 5, 7
    fb = model.sizes(h, w)[2]
    data = np.random.default_rng(4).integers(0, 256, 3 * fb + fb // 2, dtype=np.uint8)

    class Dribble(io.BytesIO):                                  # a pipe may return less than asked for
        def read(self, n=-1):
            return super().read(min(n, 11) if n and n > 0 else n)
    for stream in (io.BytesIO(data.tobytes()), Dribble(data.tobytes())):
        frames = list(pc.iter_yuv420(stream, w, h, bits=10))
        assert len(frames) == 3 and all(f.shape == (fb,) and f.dtype == np.uint8 for f in frames)
        assert np.array_equal(np.concatenate(frames), data[:3 * fb])
    assert len(list(pc.iter_yuv420(io.BytesIO(data.tobytes()), w, h))) == 7             # the default is 8-bit, as it was
    with pytest.raises(ValueError):
        next(pc.iter_yuv420(io.BytesIO(b""), w, h, bits=12))


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------------------

FAMILIES = ("unpack10", "egress10")


def test_header_prototypes_are_the_bound_symbols():
    """include/crtfx_deep.h declares exactly _lib.DEEP_SYMBOLS (argument counts included): two families of seven that mirror crtfx_unpack_* /
    crtfx_egress_* signature for signature; the table is disjoint from the other four; both new files are sources of the build; the built
    library exports every symbol."""
    hdr = open(os.path.join(ROOT, "include", "crtfx_deep.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(crtfx_(?:unpack10|egress10)_\w+)\s*\(([^)]*)\)\s*;", hdr)}
    assert set(protos) == set(_lib.DEEP_SYMBOLS) and len(protos) == 14, set(protos) ^ set(_lib.DEEP_SYMBOLS)
    assert not set(_lib.DEEP_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.INGEST_SYMBOLS) | set(_lib.EGRESS_SYMBOLS) | set(_lib.UNPACK_SYMBOLS))
    for name, args in protos.items():
        n_args = 0 if args.strip() in ("", "void") else len(args.split(","))
        assert n_args == len(_lib.DEEP_SYMBOLS[name][1]), name
        assert _lib.DEEP_SYMBOLS[name] == _lib.UNPACK_SYMBOLS[name.replace("crtfx_unpack10_", "crtfx_unpack_").replace("crtfx_egress10_", "crtfx_unpack_")], name
    assert re.search(r"CRTFX_DEEP_YUV420P10LE\s*=\s*0\s*,\s*CRTFX_DEEP_P010LE\s*=\s*1", hdr)
    assert (_lib.DEEP_YUV420P10LE, _lib.DEEP_P010LE, _lib.UNPACK10_OPT_FORCE_GENERAL, _lib.EGRESS10_OPT_FORCE_GENERAL) == (0, 1, 1, 1)
    assert all(os.path.basename(f) in {os.path.basename(s) for s in _lib.SOURCES} for f in ("crtfx_deep.hip", "crtfx_deep.h"))
    lib = _lib.load()
    for name in _lib.DEEP_SYMBOLS:
        assert getattr(lib, name).argtypes == _lib.DEEP_SYMBOLS[name][1]
    import pythoncrt_amd as pc
    assert pc.UnpackYuv10.__name__ in pc.__all__ and pc.EgressYuv10.__name__ in pc.__all__


def _table(fam):
    return tables.rgb_matrix10 if fam == "unpack10" else tables.yuv_matrix10


def _create(lib, fam, h=12, w=20, pix_fmt=_lib.PIX_F16, layout=_lib.DEEP_P010LE, device=0, m=None, off=None, null=False):
    tm, toff = _table(fam)("bt601", "tv")
    m = tm if m is None else np.ascontiguousarray(m, dtype=np.int32)
    off = toff if off is None else np.ascontiguousarray(off, dtype=np.int32)
    plan = ctypes.c_void_p(1)
    rc = getattr(lib, f"crtfx_{fam}_create")(device, h, w, pix_fmt, layout, None if null else tables.ptr(m), tables.ptr(off), ctypes.byref(plan))
    return rc, plan, (getattr(lib, f"crtfx_{fam}_last_error")(None) or b"").decode()


@pytest.mark.parametrize("fam", FAMILIES)
def test_create_refuses_bad_arguments_before_it_touches_a_device(fam):
    """The argument checks come first, so they hold on any machine: uint8 frames are UNSUPPORTED and the message names half; a size < 1 or
    > 32767, an unknown layout or pixel format, a null table, an offset of 1024 and a matrix whose accumulator could overflow are INVALID;
    each leaves *out_plan NULL and a message."""
    lib = _lib.load()
    good = _table(fam)("bt601", "tv")[0]
    too_big, too_negative = good.copy(), good.copy()
    if fam == "unpack10":
        too_big[0] = 1 << 21                                  # R row: 1023 * (2^21 + 104597) + 2^15 passes 2^31
        too_negative[4] = -(1 << 21)                          # G row: the rule sums magnitudes
        fits = good.copy()
        fits[0:3] = (2099169, 0, 0)                           # 1023 * 2099169 + 2^15 = 2^31 - 993: admitted (2099170 is not)
    else:
        too_big[0] = 1 << 21                                  # Y row: 1020 * 2^21 passes 2^31
        too_negative[4] = -40000                              # U row: 2^27 + 2^17 - 4080 * (9714 + 40000) < 0
        fits = good.copy()
        fits[0:3] = (2101231, 0, 0)                           # 1020 * 2101231 + 64 * 2^16 + 2^15 = 2^31 - 956: admitted (2101232 is not)
    over = fits.copy()
    over[0] += 1
    assert (1023 * 2099169 + (1 << 15), 1020 * 2101231 + (64 << 16) + (1 << 15)) == (2 ** 31 - 993, 2 ** 31 - 956)
    cases = [(dict(m=over), _lib.E_INVALID, "accumulator"), (dict(pix_fmt=_lib.PIX_U8), _lib.E_UNSUPPORTED, "half"), (dict(h=0), _lib.E_INVALID, "size"), (dict(w=0), _lib.E_INVALID, "size"),
             (dict(w=40000), _lib.E_INVALID, "size"), (dict(h=32768), _lib.E_INVALID, "size"), (dict(null=True), _lib.E_INVALID, "null"),
             (dict(pix_fmt=7), _lib.E_INVALID, "pixel format"), (dict(layout=2), _lib.E_INVALID, "layout"), (dict(layout=-1), _lib.E_INVALID, "layout"),
             (dict(off=(64, 1024, 512)), _lib.E_INVALID, "offset"), (dict(off=(-1, 512, 512)), _lib.E_INVALID, "offset"),
             (dict(m=too_big), _lib.E_INVALID, "accumulator"), (dict(m=too_negative), _lib.E_INVALID, "accumulator")]
    for kw, code, word in cases:
        rc, plan, msg = _create(lib, fam, **kw)
        assert rc == code and not plan.value and word in msg, (kw, rc, plan.value, msg)
    for kw in (dict(m=fits), dict(off=(1023, 0, 1023)) if fam == "unpack10" else dict(off=(64, 512, 512))):
        rc, plan, msg = _create(lib, fam, **kw)
        assert rc in (_lib.OK, _lib.E_HIP), (kw, rc, msg)         # no device here: E_HIP; with one: a plan
        if rc == _lib.OK:
            assert getattr(lib, f"crtfx_{fam}_destroy")(plan) == _lib.OK
    f = lambda name: getattr(lib, f"crtfx_{fam}_{name}")          # noqa: E731
    assert f("destroy")(None) == _lib.OK and f("set_option")(None, 1, 1) == _lib.E_INVALID
    assert f("run")(None, None, 0, None, 0, 1, None) == _lib.E_INVALID and f("frame_bytes")(None) == 0
    assert f("last_plan")(None, ctypes.create_string_buffer(8), 8) == _lib.E_INVALID


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
    """Exactly eight kernel builds (two directions x two paths x two layouts) in the library's code objects (tools/kernel_resources.py): no
    spills, no scratch memory, no LDS, and at most 128 VGPRs + AGPRs (four waves per SIMD).  Not 64 as the 8-bit stages assert: the egress
    vec build holds 2 x 12 input dwords and passes it.  include/crtfx_deep.h states the counts the build shows."""
    import kernel_resources
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    res = kernel_resources.resources(_lib.LIB_PATH)
    found = {n: v for n, v in res.items() if n.startswith("crtfx_deep_impl::")}
    kinds = [f"k_{d}10_420_{p}" for d in ("unpack", "egress") for p in ("vec", "general")]
    assert set(found) == {f"crtfx_deep_impl::{k}<{l}>" for k in kinds for l in ("true", "false")}, sorted(found)
    hdr = open(os.path.join(ROOT, "include", "crtfx_deep.h")).read()
    line = re.search(r"k_unpack10_420_vec \d+ VGPRs[^;]*;", hdr, flags=re.S)
    assert line, "the header's register line"
    stated = {k: {int(x) for x in re.findall(r"\b(\d+)\b", seg)} for k, seg in re.findall(r"(k_\w+10_420_\w+) ([^k;]*)", line.group(0))}
    for name, v in found.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["group_segment_fixed_size"] == 0 and v["vgpr_count"] + v["agpr_count"] <= 128, (name, v)
    for k in kinds:
        built = {found[f"crtfx_deep_impl::{k}<{l}>"]["vgpr_count"] + found[f"crtfx_deep_impl::{k}<{l}>"]["agpr_count"] for l in ("true", "false")}
        assert stated[k] == built, (k, stated[k], built)


# ---- refusals that need no device -----------------------------------------------------------------------------------------------------------

def test_process_frames_refuses_before_it_touches_a_device():
    """A 10-bit format on one end only, an in_size other than the output size and resize_on="host": ValueError, each message names its
    reason, no frame is read and nothing is written (they hold on a machine without a GPU)."""
    import pythoncrt_amd as pc

    def never():
        raise AssertionError("a frame was read")
        yield

    def call(**kw):
        return pc.process_frames(never(), lambda a: (_ for _ in ()).throw(AssertionError("written")), 64, 36, 30.0, 1, **kw)
    for kw, word in ((dict(in_pix_fmt="p010le"), "one end"), (dict(out_pix_fmt="yuv420p10le"), "one end"),
                     (dict(in_pix_fmt="yuv420p10le", out_pix_fmt="nv12"), "one end"), (dict(in_pix_fmt="yuv420p", out_pix_fmt="p010le"), "one end"),
                     (dict(in_pix_fmt="p010le", out_pix_fmt="p010le", in_size=(18, 32)), "in_size"),
                     (dict(in_pix_fmt="p010le", out_pix_fmt="yuv420p10le", resize_on="host"), "host"),
                     (dict(in_pix_fmt="yuv420p12le", out_pix_fmt="p010le"), "in_pix_fmt must be 'rgb24', 'yuv420p' or 'nv12'"),
                     (dict(in_pix_fmt="p010le", out_pix_fmt="p016le"), "out_pix_fmt must be 'rgb24', 'yuv420p' or 'nv12'")):
        with pytest.raises(ValueError) as e:
            call(**kw)
        assert word in str(e.value), (kw, str(e.value))


def test_cli_refuses_before_it_touches_a_device(monkeypatch, tmp_path):
    """One end only: SystemExit that names both flags.  The sharded CLI refuses the 10-bit formats as it refuses the 8-bit 4:2:0 ones."""
    from pythoncrt_amd import cli
    src = tmp_path / "in.yuv"
    src.write_bytes(bytes(8 * 8 * 3))
    base = ["--input", str(src), "--output", str(tmp_path / "out.yuv"), "--width", "8", "--height", "8"]
    for extra in (["--in-pix-fmt", "p010le"], ["--out-pix-fmt", "yuv420p10le"], ["--in-pix-fmt", "yuv420p10le", "--out-pix-fmt", "nv12"]):
        with pytest.raises(SystemExit) as e:
            cli.main(base + extra)
        assert e.value.code not in (0, None) and "one end" in str(e.value) and "--in-pix-fmt" in str(e.value) and "--out-pix-fmt" in str(e.value)
        assert not (tmp_path / "out.yuv").exists()
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit) as e:
        cli.main(base + ["--in-pix-fmt", "p010le", "--out-pix-fmt", "p010le"])
    assert "p010le" in str(e.value) and "sharded" in str(e.value) and not (tmp_path / "out.yuv").exists()
    a = cli.add_input_flags(cli.add_output_flags(cli.build_parser())).parse_args(["--input", "x", "--in-pix-fmt", "p010le", "--out-pix-fmt", "yuv420p10le"])
    assert (a.in_pix_fmt, a.out_pix_fmt) == ("p010le", "yuv420p10le")
