"""The PAL composite-video stage without a GPU (include/crtfx_pal.h): the model against a per-pixel restatement of the header, the two matrices
and their exact round trip, its properties (flat colours survive at theta = 0, the period of four frames, DELAY as the mean of SIMPLE over a
row and its partner, the row-0 rule, the phase table, the int16 / int32 bounds, the half quantiser, the smallest widths), three pinned
scenes (a phase error under both decoders, vertical chroma resolution, cross-colour on a grey stripe), the C-ABI bound symbol for symbol
and refusing bad arguments before it touches a device, every refusal of process_frames(signal_standard=, pal_decoder=, signal_phase=) and
of the CLI's flags with its rule, PAL_RULES, the stages of SourceEnd with and without the keyword, and the builds' registers and LDS
against the header."""
import ctypes
import itertools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pythoncrt_amd import _lib, _stage, adeint, canvas, deint, depth, ends, formats, ingest, lut3d, options, resample, resize16  # noqa: E402
from pythoncrt_amd import pal as pal_mod  # noqa: E402
from pythoncrt_amd import signal as signal_mod  # noqa: E402
from tests import pal_model as model  # noqa: E402

HEADER = os.path.join(ROOT, "include", "crtfx_pal.h")
DTYPES = (np.uint8, np.float16)
COMBOS = list(itertools.product(model.SIGNALS, model.CHROMAS, model.DECODERS))


def _all_halves():
    return np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)


def _source(dtype, shape, seed):
    """Noise: bytes; or halves across every rule — quarter codes, values between them and past both ends, NaN, infinities, -0."""
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    f = (rng.integers(-40, 8 * 1030, shape) / 32.0).astype(np.float16)
    flat = f.reshape(-1)
    pick = rng.integers(0, flat.size, max(1, flat.size // 16))
    flat[pick] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0, 255.5, 254.875, 0.125, 6e-8, 65504.0], dtype=np.float16), pick.size)
    return f


def _extremes(dtype, shape, seed):
    """{0, M} noise."""
    return (np.random.default_rng(seed).integers(0, 2, shape) * 255).astype(dtype)


# ---- the arithmetic -------------------------------------------------------------------------------------------------------------------------

def _code(sample):
    """One sample's integer, from the header's words (not through the model)."""
    if isinstance(sample, np.uint8):
        return int(sample)
    f = float(sample)
    if f != f:
        return 0
    t = min(max(4.0 * f, 0.0), 1020.0)
    lo = int(np.floor(t))
    frac = t - lo
    return lo + (1 if frac > 0.5 or (frac == 0.5 and lo % 2 == 1) else 0)


COS, SIN = (1, 0, -1, 0), (0, 1, 0, -1)


def _per_pixel(frames, signal, chroma, crawl, index, decoder, phase):
    """The header, one sample at a time: every quantity a function of x on the extended row of row y."""
    import math
    n, h, w, _ = frames.shape
    half = frames.dtype == np.float16
    top = 1020 if half else 255
    out = np.zeros(frames.shape, dtype=frames.dtype)
    D, shift = (([1, 2, 3, 4, 3, 2, 1], 4) if chroma == "sharp" else (list(range(1, 9)) + list(range(7, 0, -1)), 6))
    r = len(D) // 2
    T7 = [1, 2, 3, 4, 3, 2, 1]
    c = 1 if crawl else 0
    ct, st = round(4096 * math.cos(math.radians(phase))), round(4096 * math.sin(math.radians(phase)))
    for f in range(n):
        t = index + f
        memo = {}

        def ph(x, y):
            return (x + 3 * y + 3 * c * t) % 4                                   # Python's % is non-negative

        def v(y):
            return 1 if (y + c * t) % 2 == 0 else -1

        def yuv(x, y):
            if (x, y) not in memo:
                R, G, B = (_code(frames[f, y, min(max(x, 0), w - 1), k]) for k in range(3))
                memo[x, y] = ((1225 * R + 2404 * G + 467 * B + 128) >> 8, (-603 * R - 1183 * G + 1786 * B + 128) >> 8,
                              (2518 * R - 2109 * G - 409 * B + 128) >> 8)
            return memo[x, y]

        def C(x, y):
            u1 = (sum(T7[k + 3] * yuv(x + k, y)[1] for k in range(-3, 4)) + 8) >> 4
            v1 = (sum(T7[k + 3] * yuv(x + k, y)[2] for k in range(-3, 4)) + 8) >> 4
            return u1 * SIN[ph(x, y)] + v(y) * v1 * COS[ph(x, y)]

        def s(x, y):
            return yuv(x, y)[0] + C(x, y)

        def Yd(x, y):
            return (s(x - 2, y) + 2 * s(x, y) + s(x + 2, y) + 2) >> 2 if signal == "composite" else yuv(x, y)[0]

        def e(x, y):
            return s(x, y) - Yd(x, y) if signal == "composite" else C(x, y)

        def rotated(x, y):
            ud = (sum(D[k + r] * 2 * e(x + k, y) * SIN[ph(x + k, y)] for k in range(-r, r + 1)) + (1 << (shift - 1))) >> shift
            vd = (sum(D[k + r] * 2 * e(x + k, y) * v(y) * COS[ph(x + k, y)] for k in range(-r, r + 1)) + (1 << (shift - 1))) >> shift
            return (ct * ud + v(y) * st * vd + 2048) >> 12, (ct * vd - v(y) * st * ud + 2048) >> 12
        for y in range(h):
            yp = y - 1 if y >= 1 else (1 if h > 1 else 0)
            for x in range(w):
                U, V = rotated(x, y)
                if decoder == "delay":
                    up, vp = rotated(x, yp)
                    U, V = (U + up + 1) >> 1, (V + vp + 1) >> 1
                yd = Yd(x, y)
                rgb = ((4096 * yd + 4670 * V + 32768) >> 16, (4096 * yd - 1617 * U - 2379 * V + 32768) >> 16, (4096 * yd + 8325 * U + 32768) >> 16)
                for k in range(3):
                    q = min(max(rgb[k], 0), top)
                    out[f, y, x, k] = np.float16(q / 4.0) if half else q
    return out


def test_names_are_one_list_in_the_model_and_the_module():
    assert pal_mod.DECODERS == model.DECODERS == ("delay", "simple") and pal_mod.PHASES == (-180, 180)
    assert signal_mod.SIGNALS == model.SIGNALS == ("composite", "svideo") and signal_mod.CHROMAS == model.CHROMAS == ("sharp", "soft")
    assert pal_mod.PalSignal.frames_in == 1 and pal_mod.PalSignal.frames_out == 1 and pal_mod.STRIP in (8, 16, 32)
    assert (_lib.PAL_DELAY, _lib.PAL_SIMPLE) == (0, 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("signal,chroma,decoder", COMBOS)
def test_model_against_the_header_per_pixel(dtype, signal, chroma, decoder):
    """Widths from 1 (every tap is the edge pixel), heights 1 to 4 (the row-0 rule, both V switches), crawl on and off, every index mod 4,
    phase errors of both signs."""
    for (h, w), n, crawl, index, phase in (((1, 1), 2, True, 0, 20), ((2, 2), 1, False, 3, -90), ((1, 3), 2, True, 1, 0), ((3, 5), 2, True, 2, 180),
                                           ((2, 5), 2, False, 1, -33), ((4, 19), 1, True, 3, 71)):
        src = _source(dtype, (n, h, w, 3), [h, w, n])
        got = model.pal(src, signal, chroma, crawl, index, decoder, phase)
        assert got.dtype == dtype and got.shape == src.shape
        assert np.array_equal(model.bits(got), model.bits(_per_pixel(src, signal, chroma, crawl, index, decoder, phase))), (h, w, n, crawl, index, phase)
    ext = _extremes(dtype, (1, 3, 9, 3), 5)
    assert np.array_equal(model.bits(model.pal(ext, signal, chroma, True, 1, decoder, 45)), model.bits(_per_pixel(ext, signal, chroma, True, 1, decoder, 45)))
    assert model.pal(src[:0], signal, chroma, decoder=decoder).shape == (0, 4, 19, 3)


def test_the_two_matrices_are_the_headers_literals():
    assert model.TO_YUV.tolist() == [[1225, 2404, 467], [-603, -1183, 1786], [2518, -2109, -409]]
    assert model.TO_RGB.tolist() == [[4096, 0, 4670], [4096, -1617, -2379], [4096, 8325, 0]]
    assert model.TO_YUV[0].sum() == 4096 and model.TO_YUV[1].sum() == 0 and model.TO_YUV[2].sum() == 0       # grey has no chroma
    hdr = open(HEADER).read()
    for text in ("(1225 R + 2404 G +  467 B + 128) >> 8", "(-603 R - 1183 G + 1786 B + 128) >> 8", "(2518 R - 2109 G -  409 B + 128) >> 8",
                 "(4096 Yd + 4670 V + 32768) >> 16", "(4096 Yd - 1617 U - 2379 V + 32768) >> 16", "(4096 Yd + 8325 U + 32768) >> 16"):
        assert text in hdr, text


def _round_trip(cols):
    """Steps 1 and 9 on colours [m, 3], in int32."""
    c = cols.astype(np.int32)
    y, u, v = ((np.int32(m[0]) * c[:, 0] + np.int32(m[1]) * c[:, 1] + np.int32(m[2]) * c[:, 2] + np.int32(128)) >> 8 for m in model.TO_YUV)
    return np.stack([(np.int32(m[0]) * y + np.int32(m[1]) * u + np.int32(m[2]) * v + np.int32(32768)) >> 16 for m in model.TO_RGB], axis=-1)


def test_the_matrix_pair_returns_every_byte_triple_and_a_sample_of_quarter_code_triples():
    g = np.arange(256, dtype=np.int32)
    gb = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    for r0 in range(0, 256, 16):
        cols = np.concatenate([np.concatenate([np.full((gb.shape[0], 1), r, dtype=np.int32), gb], axis=1) for r in range(r0, r0 + 16)])
        assert np.array_equal(_round_trip(cols), cols), r0
    q = np.random.default_rng(11).integers(0, 1021, (1 << 20, 3))
    assert np.array_equal(_round_trip(q), q)
    corners = np.array(list(itertools.product((0, 1, 510, 1019, 1020), repeat=3)))
    assert np.array_equal(_round_trip(corners), corners)


def test_a_flat_colour_returns_itself_at_theta_0():
    """Under both signals, both filters and both decoders, at t = 0..3: bytes and quarter codes."""
    rng = np.random.default_rng(12)
    for top in (255, 1020):
        cols = np.concatenate([rng.integers(0, top + 1, (4096, 3)), np.array(list(itertools.product((0, 1, top // 2, top - 1, top), repeat=3)))])
        c = np.broadcast_to(cols[:, None, None, :], (cols.shape[0], 3, 4, 3)).astype(np.int64)
        for signal, chroma, decoder in COMBOS:
            for t in range(4):
                assert np.array_equal(model.cascade(c, signal, chroma, True, t, decoder, 0), c), (signal, chroma, decoder, t)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("chroma", model.CHROMAS)
@pytest.mark.parametrize("decoder", model.DECODERS)
def test_the_period_of_four_frames(dtype, chroma, decoder):
    """Under composite with crawl: t and t + 4 give the same bytes, t and t + 1 do not; without crawl t does not matter; a frame later is a
    line later away from the top rows."""
    src = _source(dtype, (1, 6, 40, 3), 13)
    outs = [model.bits(model.pal(src, "composite", chroma, True, t, decoder, 20)) for t in range(9)]
    for t in range(5):
        assert np.array_equal(outs[t], outs[t + 4]) and not np.array_equal(outs[t], outs[t + 1]), t
    assert len({o.tobytes() for o in outs[:4]}) == 4
    still = [model.bits(model.pal(src, "composite", chroma, False, t, decoder, 20)) for t in range(3)]
    assert np.array_equal(still[0], still[1]) and np.array_equal(still[0], still[2]) and np.array_equal(still[0], outs[0])
    rows = np.repeat(_source(dtype, (1, 1, 40, 3), 14), 7, axis=1)                # rows of equal content
    a, b = (model.bits(model.pal(rows, "composite", chroma, True, t, decoder, 20)) for t in (0, 1))
    assert np.array_equal(b[0, 2:-1], a[0, 3:])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("signal,chroma", list(itertools.product(model.SIGNALS, model.CHROMAS)))
def test_delay_is_simple_averaged_over_a_row_and_its_partner(dtype, signal, chroma):
    """At theta = 0 (and at any other): U and V of DELAY are the stated rounded means of SIMPLE's over (y, y'), and Yd is SIMPLE's."""
    for h, phase in ((1, 0), (2, 0), (3, 0), (5, 0), (4, 33)):
        c = model.codes(_source(dtype, (2, h, 21, 3), [h, 15]))
        simple, delay = [], []
        model.cascade(c, signal, chroma, True, 1, "simple", phase, uv=simple)
        out = model.cascade(c, signal, chroma, True, 1, "delay", phase, uv=delay)
        (us, vs), (ud, vd) = simple[0], delay[0]
        yp = [max(y - 1, 0) if y else min(1, h - 1) for y in range(h)]
        assert np.array_equal(ud, (us + us[:, yp] + 1) >> 1) and np.array_equal(vd, (vs + vs[:, yp] + 1) >> 1)
        yd, _, _ = model.rows(c, signal, chroma, True, 1, phase)
        assert np.array_equal(out, np.stack([m[0] * yd + m[1] * ud + m[2] * vd + 32768 for m in model.TO_RGB], axis=-1) >> 16)


def test_the_row_0_rule():
    assert [model.partner_rows(h).tolist() for h in (1, 2, 3, 5)] == [[0], [1, 0], [1, 0, 1], [1, 0, 1, 2, 3]]
    src = _source(np.uint8, (1, 3, 24, 3), 16)
    for h in (1, 2, 3):
        got = model.pal(src[:, :h], "svideo", "sharp", True, 0, "delay", 0)
        uv = []
        model.cascade(model.codes(src[:, :h]), "svideo", "sharp", True, 0, "simple", 0, uv=uv)
        u = uv[0][0][0]
        if h == 1:                                                              # its own partner: DELAY is SIMPLE
            assert np.array_equal(got, model.pal(src[:, :1], "svideo", "sharp", True, 0, "simple", 0))
        else:                                                                   # rows 0 and 1 are each other's partner: the same U and V
            d = []
            model.cascade(model.codes(src[:, :h]), "svideo", "sharp", True, 0, "delay", 0, uv=d)
            assert np.array_equal(d[0][0][0, 0], d[0][0][0, 1]) and np.array_equal(d[0][0][0, 0], (u[0] + u[1] + 1) >> 1)
            assert not np.array_equal(got[0, 0], model.pal(src[:, :1], "svideo", "sharp", True, 0, "delay", 0)[0, 0])
        if h == 3:
            assert np.array_equal(d[0][0][0, 2], (u[2] + u[1] + 1) >> 1)


def test_the_phase_table_for_all_361_degrees():
    import math
    lib = _lib.load()
    c, s = ctypes.c_int(), ctypes.c_int()
    worst = 1.0
    for deg in range(-180, 181):
        assert lib.crtfx_pal_phase_table(deg, ctypes.byref(c), ctypes.byref(s)) == _lib.OK
        assert (c.value, s.value) == model.phase_table(deg) == pal_mod.phase_table(deg), deg
        for f in (4096 * math.cos(math.radians(deg)), 4096 * math.sin(math.radians(deg))):
            worst = min(worst, abs(abs(f - math.floor(f)) - 0.5))
    assert worst > 0.004                                                        # no integer degree comes near a rounding tie
    assert model.phase_table(0) == (4096, 0) and model.phase_table(90) == (0, 4096) and model.phase_table(-90) == (0, -4096)
    assert model.phase_table(180) == model.phase_table(-180) == (-4096, 0) and model.phase_table(20) == (3849, 1401)
    assert max(abs(a) + abs(b) for a, b in map(model.phase_table, range(-180, 181))) == 5792
    for bad in (-181, 181, 1000):
        assert lib.crtfx_pal_phase_table(bad, ctypes.byref(c), ctypes.byref(s)) == _lib.E_INVALID
    assert lib.crtfx_pal_phase_table(0, None, ctypes.byref(s)) == _lib.E_INVALID and lib.crtfx_pal_phase_table(0, ctypes.byref(c), None) == _lib.E_INVALID
    for bad in (True, 1.0, "20", None, 181):
        with pytest.raises(ValueError, match="phase"):
            pal_mod.check_phase(bad)


def test_the_int16_and_int32_bounds_by_the_sum_of_absolute_values():
    """On quarter codes, the wider scale, as the header derives them — and they hold its figures."""
    m = model.TO_YUV
    pos, neg = np.where(m > 0, m, 0).sum(axis=1), np.where(m < 0, m, 0).sum(axis=1)
    hi, lo = (pos * 1020 + 128) >> 8, (neg * 1020 + 128) >> 8
    assert list(hi) == [16320, 7116, 10033] and list(lo) == [0, -7116, -10033]
    bytes_hi = (pos * 255 + 128) >> 8
    assert list(bytes_hi[1:]) == [1779, 2508]
    s_lo, s_hi = int(lo[2]), int(hi[0] + hi[2])
    assert (s_lo, s_hi) == (-10033, 26353) and -32768 <= s_lo and s_hi <= 32767
    e_max = s_hi - s_lo
    c_max = e_max + 1                                                           # 2 e over half of a filter of gain 1, and its rounding
    assert (e_max, c_max) == (36386, 36387)
    rot = 5792 * c_max + 2048
    uv_max = rot >> 12
    assert rot <= model.ROT_MAX < 2 ** 31 and uv_max == 51453
    last = int(4096 * s_hi + np.abs(model.TO_RGB[:, 1:]).sum(axis=1).max() * uv_max + 32768)
    assert last <= model.ACC_MAX < 2 ** 31 and last > 5e8                       # the header's 5.4e8 is this bound, not a loose one
    assert 64 * 2 * e_max + 32 < 2 ** 31 and int(np.abs(m).sum(axis=1).max()) * 1020 + 128 < 2 ** 31
    hdr = " ".join(open(HEADER).read().replace("\n *", " ").split())
    for text in ("|U0| <= 7116, |V0| <= 10033", "-10033 .. 26353", "|e| <= 36386", "|Ud|, |Vd| <= 36387", "<= 5792", "below 2.2e8", "<= 51453", "below 5.4e8"):
        assert text in hdr, text


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("signal,chroma,decoder", COMBOS)
def test_the_bounds_hold_on_extreme_noise_and_on_the_frames_that_drive_them(dtype, signal, chroma, decoder):
    """{0, M} noise, and stripes of period 4 and 2 between saturated colours at the carrier's own frequency: both clamps are driven, the
    planes stay inside int16 and the accumulators under the header's bounds; a red and a blue frame attain the bounds of V0 and U0."""
    top = model.top(dtype)
    acc = {}
    src = _extremes(dtype, (2, 8, 64, 3), 21)
    v = model.cascade(model.codes(src), signal, chroma, True, 0, decoder, 45, acc)
    out = model.codes(model.pal(src, signal, chroma, True, 0, decoder, 45))
    assert (v < 0).any() and (v > top).any() and out.min() == 0 and out.max() == top and np.mean(out != model.codes(src)) > 0.5
    prim = [(top, 0, 0), (0, top, 0), (0, 0, top), (top, top, 0), (0, top, top), (top, 0, top), (0, 0, 0), (top, top, top)]
    for a, b in itertools.permutations(prim, 2):
        for period in (2, 4):
            c = np.zeros((4, 4, 32, 3), dtype=np.int64)
            c[:, :, (np.arange(32) % period) < period // 2] = a
            c[:, :, (np.arange(32) % period) >= period // 2] = b
            model.cascade(c, signal, chroma, True, 0, decoder, 45, acc)
    scale = 4 if dtype == np.uint8 else 1
    assert acc["u0"] * scale <= 7116 + 3 and acc["v0"] * scale <= 10033 + 3 and acc["y0"] <= 16320
    assert (acc["u0"], acc["v0"]) == ((1779, 2508) if dtype == np.uint8 else (7116, 10033))
    assert -10033 <= acc["s_min"] and acc["s_max"] <= 26353 and acc["e"] <= 36386 and acc["ud"] <= 36387
    assert acc["rot"] <= model.ROT_MAX and acc["uv"] <= 51453 and acc["last"] <= model.ACC_MAX
    print(f"{signal} {chroma} {decoder} {np.dtype(dtype).name}: {acc}")


def test_the_half_quantiser_on_every_pattern():
    h = _all_halves()
    q = model.quantise(h)
    assert q.min() == 0 and q.max() == 1020 and np.array_equal(q, np.array([_code(v) for v in h]))
    frames = np.resize(h, (1, 16, 1366, 3))
    assert np.array_equal(np.unique(model.bits(frames)), np.arange(65536))
    for signal, chroma, decoder in (("composite", "sharp", "delay"), ("svideo", "soft", "simple")):
        out = model.pal(frames, signal, chroma, decoder=decoder, phase=20)
        assert np.array_equal(model.bits(out), model.bits(model.pal(model.from_codes(model.quantise(frames), np.float16), signal, chroma, decoder=decoder, phase=20)))
        assert np.isfinite(out.astype(np.float32)).all() and np.array_equal(model.quantise(out).astype(np.float64) / 4.0, out.astype(np.float64))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_smallest_widths(dtype):
    """Widths 1 to 5 at heights 1 to 3: narrower than every filter, so every tap is an edge pixel; a row of one pixel is a flat colour,
    which survives where theta = 0."""
    for signal, chroma, decoder in COMBOS:
        for h, w in itertools.product((1, 2, 3), (1, 2, 3, 4, 5)):
            src = _source(dtype, (3, h, w, 3), [h, w])
            out = model.pal(src, signal, chroma, True, 2, decoder, 20)
            assert out.shape == src.shape and out.dtype == dtype
            if w == 1 and (h == 1 or decoder == "simple"):
                assert np.array_equal(model.codes(model.pal(src, signal, chroma, True, 2, decoder, 0)), model.codes(src))
            wide = np.concatenate([np.repeat(src[:, :, :1], 12, axis=2), src, np.repeat(src[:, :, -1:], 12, axis=2)], axis=2)
            assert np.array_equal(model.bits(model.pal(wide, signal, chroma, True, 2, decoder, 20)[:, :, 12:12 + w]), model.bits(out))


# ---- three pinned scenes ------------------------------------------------------------------------------------------------------------------------

def test_scene_a_phase_error_desaturates_under_delay_and_shows_hanover_bars_under_simple():
    src = np.zeros((1, 6, 24, 3), dtype=np.uint8)
    src[...] = (200, 60, 90)
    d = model.pal(src, "composite", "sharp", True, 0, "delay", 20)
    assert (d == np.array([194, 63, 91], dtype=np.uint8)).all()                # Y + (C - Y) cos 20: 194.29, 62.73, 90.92
    s = model.pal(src, "composite", "sharp", True, 0, "simple", 20)
    assert (s[:, 0::2] == np.array([197, 50, 149], dtype=np.uint8)).all() and (s[:, 1::2] == np.array([191, 75, 33], dtype=np.uint8)).all()
    y = (1225 * 200 + 2404 * 60 + 467 * 90) / 4096.0
    assert [round(y + (c - y) * np.cos(np.radians(20))) for c in (200, 60, 90)] == [194, 63, 91]


def test_scene_vertical_chroma_resolution_is_halved_under_delay():
    src = np.zeros((1, 8, 24, 3), dtype=np.uint8)
    src[:, 0::2] = (255, 0, 0)
    src[:, 1::2] = (0, 0, 255)
    d = model.pal(src, "svideo", "sharp", True, 0, "delay", 0)
    assert (d[0, 0::2, 10] == np.array([151, 24, 151], dtype=np.uint8)).all() and (d[0, 1::2, 10] == np.array([104, 0, 104], dtype=np.uint8)).all()
    assert np.array_equal(model.pal(src, "svideo", "sharp", True, 0, "simple", 0), src)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("chroma", model.CHROMAS)
def test_scene_a_grey_stripe_of_period_4_comes_back_coloured_and_less_so_under_delay(dtype, chroma):
    top = model.top(dtype)
    stripe = np.zeros((1, 8, 64, 3), dtype=np.int64)
    stripe[:, :, (np.arange(64) % 4) < 2, :] = top                              # two pixels on, two off: luma detail AT the subcarrier
    energy = {}
    for decoder in model.DECODERS:
        uv = []
        out = np.clip(model.cascade(stripe, "composite", chroma, True, 0, decoder, 0, uv=uv), 0, top)
        assert int((out.max(axis=-1) - out.min(axis=-1)).max()) > top // 4      # coloured
        energy[decoder] = int(np.abs(uv[0][0]).sum() + np.abs(uv[0][1]).sum())
        assert np.array_equal(np.clip(model.cascade(stripe, "svideo", chroma, True, 0, decoder, 0), 0, top), stripe)     # no crosstalk without the sum
    print(f"{np.dtype(dtype).name} {chroma}: summed |U| + |V| {energy}")
    assert 0 < energy["delay"] < energy["simple"]


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------------------

_vp = ctypes.c_void_p
SIGNATURES = {
    "crtfx_pal_create": (ctypes.c_int, [ctypes.c_int] * 9 + [ctypes.POINTER(_vp)]),
    "crtfx_pal_destroy": (ctypes.c_int, [_vp]),
    "crtfx_pal_last_error": (ctypes.c_char_p, [_vp]),
    "crtfx_pal_run": (ctypes.c_int, [_vp, ctypes.c_int64, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_int, _vp]),
    "crtfx_pal_set_option": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "crtfx_pal_last_plan": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_size_t]),
    "crtfx_pal_phase_table": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
}


def test_symbols_are_bound_and_the_header_declares_them():
    assert _lib.PAL_SYMBOLS == SIGNATURES and list(_lib.PAL_SYMBOLS) == list(SIGNATURES) and _lib.PAL_OPT_FORCE_GENERAL == 1
    assert _lib.PAL_SYMBOLS == _lib.frame_symbols("pal", [ctypes.c_int] * 8, run=SIGNATURES["crtfx_pal_run"], phase_table=SIGNATURES["crtfx_pal_phase_table"])
    lib = _lib.load()
    for name, (res, args) in SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res, name
    hdr = open(HEADER).read()
    flat = " ".join(hdr.replace("\n *", " ").split())
    for text in ("CRTFX_PAL_OPT_FORCE_GENERAL = 1", "CRTFX_PAL_COMPOSITE = 0", "CRTFX_PAL_SVIDEO = 1", "CRTFX_PAL_SHARP = 0", "CRTFX_PAL_SOFT = 1",
                 "CRTFX_PAL_DELAY = 0", "CRTFX_PAL_SIMPLE = 1", "NOT claimed is equality with any other PAL implementation",
                 "pal=k_pal<composite,soft,delay,u8,vec>;frames=5", "no 25 Hz offset", "no RF noise", "taken as consecutive lines", "NTSC has no phase knob"):
        assert text in flat, text
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(crtfx_pal_\w+)\s*\(([^)]*)\)\s*;", hdr)}
    assert set(protos) == set(SIGNATURES) and len(protos) == 7, set(protos) ^ set(SIGNATURES)
    for name, args in protos.items():
        assert len(args.split(",")) == len(SIGNATURES[name][1]), name
    order = [a.split()[-1].lstrip("*") for a in protos["crtfx_pal_create"].split(",")]
    assert order == ["device", "h", "w", "pix_fmt", "signal", "chroma", "crawl", "decoder", "phase", "out_plan"]
    order = [a.split()[-1].lstrip("*") for a in protos["crtfx_pal_run"].split(",")]
    assert order[:2] == ["plan", "first_index"] and "int64_t first_index" in protos["crtfx_pal_run"]
    assert [a.split()[-1].lstrip("*") for a in protos["crtfx_pal_phase_table"].split(",")] == ["degrees", "c", "s"]
    others = set()
    for table in ("SYMBOLS", "INGEST_SYMBOLS", "EGRESS_SYMBOLS", "UNPACK_SYMBOLS", "DEEP_SYMBOLS", "YUV422_SYMBOLS", "DEEP444_SYMBOLS", "SITED_SYMBOLS",
                  "EGRESS_SITED_SYMBOLS", "FIELD420_SYMBOLS", "EGRESS_FIELD420_SYMBOLS", "RESIZE16_SYMBOLS", "RESAMPLE_SYMBOLS", "CANVAS_SYMBOLS",
                  "DEPTH_SYMBOLS", "DEINT_SYMBOLS", "ADEINT_SYMBOLS", "LUT3D_SYMBOLS", "INTERLACE_SYMBOLS", "SIGNAL_SYMBOLS", "PROBE_SYMBOLS"):
        others |= set(getattr(_lib, table))
    assert not set(SIGNATURES) & others
    assert all(os.path.basename(f) in {os.path.basename(s) for s in _lib.SOURCES} for f in ("crtfx_pal.hip", "crtfx_pal.h", "crtfx_frame_host.h"))
    assert all(os.path.exists(s) for s in _lib.SOURCES) and "crtfx_pal" in _lib.STAGE_UNITS and "crtfx_signal" in _lib.STAGE_UNITS
    import pythoncrt_amd as pc
    assert pc.PalSignal is pal_mod.PalSignal and "PalSignal" in pc.__all__ and "Signal" in pc.__all__
    assert issubclass(pc.PalSignal, _stage.FramePlan) and not issubclass(pc.PalSignal, signal_mod.Signal)
    assert pc.PalSignal._family == "pal" and pc.PalSignal._force_option == 1
    unit = open(os.path.join(_lib.CSRC, "crtfx_pal.hip")).read()
    assert "namespace crtfx_pal_impl" in unit and "crtfx_frames::run<U>" in unit and "hipGetDevice" not in unit        # run() is the skeleton's
    assert "asm" not in unit and f"#define CRTFX_PAL_STRIP {pal_mod.STRIP} " in unit
    import bench                                                               # a namespace of its own, outside the chain's evidence hash
    assert "crtfx_pal" not in open(bench.__file__).read()


GOOD = dict(device=0, h=9, w=24, pix_fmt=_lib.PIX_U8, signal=_lib.SIGNAL_COMPOSITE, chroma=_lib.SIGNAL_SOFT, crawl=1, decoder=_lib.PAL_DELAY, phase=20)


def _create(lib, no_out=False, **kw):
    a = dict(GOOD)
    a.update(kw)
    plan = ctypes.c_void_p(1)
    rc = lib.crtfx_pal_create(*(a[k] for k in GOOD), None if no_out else ctypes.byref(plan))
    return rc, plan, (lib.crtfx_pal_last_error(None) or b"").decode()


def test_create_refuses_bad_arguments_before_it_touches_a_device():
    """Every refusal of crtfx_pal_create comes before the device is asked for, so it holds on any machine; *out_plan is NULL and the
    message names the offending field.  The call that passes every check is left with the device: `no HIP device 4096`."""
    lib = _lib.load()
    cases = [({k: v}, f"{k} = {v} outside 1..32767") for k in ("h", "w") for v in (0, -3, 32768)]
    cases += [({k: v}, f"unknown {k} {v}") for k in ("pix_fmt", "signal", "chroma", "decoder") for v in (2, -1, 7)]
    cases += [(dict(crawl=v), f"crawl = {v}") for v in (2, -1, 7)]
    cases += [(dict(phase=v), f"phase = {v} outside -180..180") for v in (181, -181, 360, -2 ** 31)]
    for kw, text in cases:
        rc, plan, msg = _create(lib, **kw)
        assert rc == _lib.E_INVALID and not plan.value and text in msg, (kw, rc, plan.value, msg)
    rc, plan, msg = _create(lib, no_out=True)
    assert rc == _lib.E_INVALID and "out_plan" in msg
    for kw in (dict(), dict(h=1, w=1), dict(h=32767, w=32767, pix_fmt=_lib.PIX_F16), dict(signal=1, chroma=0, crawl=0, decoder=1), dict(phase=-180),
               dict(phase=180), dict(phase=0)):
        rc, plan, msg = _create(lib, device=4096, **kw)
        assert rc == _lib.E_HIP and not plan.value and "no HIP device 4096" in msg, (kw, rc, msg)
    assert lib.crtfx_pal_destroy(None) == _lib.OK and lib.crtfx_pal_set_option(None, 1, 1) == _lib.E_INVALID
    assert lib.crtfx_pal_run(None, 0, None, 0, None, 0, 1, None) == _lib.E_INVALID
    assert lib.crtfx_pal_last_plan(None, ctypes.create_string_buffer(8), 8) == _lib.E_INVALID


def test_python_plan_refuses_before_a_device():
    for kw in (dict(signal="rf"), dict(chroma="blurry"), dict(signal=None), dict(chroma=1), dict(crawl=1), dict(crawl="on"), dict(decoder="comb"),
               dict(decoder=0), dict(decoder=None), dict(phase=181), dict(phase=-181), dict(phase=True), dict(phase=20.0), dict(phase="20")):
        with pytest.raises(ValueError, match=next(iter(kw))):
            pal_mod.PalSignal("cpu", (4, 4), **kw)
    with pytest.raises(ValueError, match="ROCm device"):
        pal_mod.PalSignal("cpu", (4, 4))
    plan = pal_mod.PalSignal.__new__(pal_mod.PalSignal)
    plan._index = 3
    for bad in (-1, 1.5, None, True):
        with pytest.raises(ValueError, match="index"):
            plan.reset(bad)
    plan.reset(6)
    assert plan._index == 6
    plan.reset()
    assert plan._index == 0
    for text in ("4 x fsc", "SD-width", "behind the stage", "no 25 Hz offset", "no RF noise", "consecutive lines"):
        assert text in " ".join((pal_mod.__doc__ + " " + pal_mod.PalSignal.__doc__).split()), text


# what include/crtfx_pal.h states for the thirty-two builds: VGPRs as built
HEADER_VGPRS = {
    "k_pal<composite,sharp,delay,u8,vec>": 85, "k_pal<composite,sharp,delay,f16,vec>": 85, "k_pal<composite,sharp,simple,u8,vec>": 70,
    "k_pal<composite,sharp,simple,f16,vec>": 68, "k_pal<composite,soft,delay,u8,vec>": 105, "k_pal<composite,soft,delay,f16,vec>": 105,
    "k_pal<composite,soft,simple,u8,vec>": 90, "k_pal<composite,soft,simple,f16,vec>": 93, "k_pal<svideo,sharp,delay,u8,vec>": 79,
    "k_pal<svideo,sharp,delay,f16,vec>": 77, "k_pal<svideo,sharp,simple,u8,vec>": 65, "k_pal<svideo,sharp,simple,f16,vec>": 61,
    "k_pal<svideo,soft,delay,u8,vec>": 103, "k_pal<svideo,soft,delay,f16,vec>": 101, "k_pal<svideo,soft,simple,u8,vec>": 85,
    "k_pal<svideo,soft,simple,f16,vec>": 88, "k_pal<composite,sharp,delay,u8,general>": 121, "k_pal<composite,sharp,delay,f16,general>": 163,
    "k_pal<composite,sharp,simple,u8,general>": 80, "k_pal<composite,sharp,simple,f16,general>": 92, "k_pal<composite,soft,delay,u8,general>": 182,
    "k_pal<composite,soft,delay,f16,general>": 232, "k_pal<composite,soft,simple,u8,general>": 112, "k_pal<composite,soft,simple,f16,general>": 167,
    "k_pal<svideo,sharp,delay,u8,general>": 96, "k_pal<svideo,sharp,delay,f16,general>": 112, "k_pal<svideo,sharp,simple,u8,general>": 61,
    "k_pal<svideo,sharp,simple,f16,general>": 67, "k_pal<svideo,soft,delay,u8,general>": 171, "k_pal<svideo,soft,delay,f16,general>": 198,
    "k_pal<svideo,soft,simple,u8,general>": 112, "k_pal<svideo,soft,simple,f16,general>": 117,
}
VEC_LDS = 4 * 4 * 528 * 2


def test_pal_kernels_have_no_scratch_and_the_headers_registers_and_lds():
    """Registers, LDS and scratch of the thirty-two builds, read from the built library's code objects (tools/kernel_resources.py): no
    scratch memory, no spills, no AGPRs, 16896 bytes of LDS for the vec builds and none for the general ones — and the figures the header
    quotes are the figures of this build.  The NTSC family's sixteen builds are its own still."""
    import kernel_resources
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    res = kernel_resources.resources(_lib.LIB_PATH)
    found = {n.replace("crtfx_pal_impl::", "").replace("crtfx_deint_impl::", "").replace(", ", ","): v
             for n, v in res.items() if n.startswith("crtfx_pal_impl::")}
    names = {f"k_pal<{s},{c},{d},{p},{path}>" for s, c, d in COMBOS for p in ("u8", "f16") for path in ("vec", "general")}
    assert set(found) == names == set(HEADER_VGPRS) and len(names) == 32, sorted(set(found) ^ names)
    hdr = open(HEADER).read()
    for name, v in found.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["group_segment_fixed_size"] == (VEC_LDS if name.endswith(",vec>") else 0) and v["agpr_count"] == 0, (name, v)
        assert v["vgpr_count"] == HEADER_VGPRS[name], (name, v["vgpr_count"])
        assert re.search(rf"{re.escape(name)} {HEADER_VGPRS[name]}\b", hdr), name
    assert f"LDS: {VEC_LDS} bytes per workgroup for every vec build" in hdr and "no AGPRs, no scratch, no spills" in hdr
    ntsc = [n for n in res if n.startswith("crtfx_signal_impl::")]
    assert len(ntsc) == 16 and all("k_signal<" in n for n in ntsc)


def test_the_ntsc_family_is_untouched():
    """include/crtfx_signal.h still says what it said, and pythoncrt_amd/signal.py knows nothing of PAL."""
    hdr = open(os.path.join(ROOT, "include", "crtfx_signal.h")).read()
    assert "NTSC-like only — no PAL, no burst-axis rotation, no RF noise" in hdr and "Sixteen builds" in hdr
    src = open(signal_mod.__file__).read()
    assert "pal" not in src.replace("no PAL", "").lower() and signal_mod.SIGNALS == ("composite", "svideo")
    assert "crtfx_pal" not in open(os.path.join(_lib.CSRC, "crtfx_signal.hip")).read()


# ---- process_frames and the CLI: every refusal comes before a device --------------------------------------------------------------------------

def _refusing_process_frames(monkeypatch):
    import torch
    import pythoncrt_amd as pc

    def never():
        raise AssertionError("a frame was read")
        yield

    def no_device():
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    return lambda h=48, **kw: pc.process_frames(never(), lambda a: None, 80, h, 30.0, 1, **kw)


def _refused(run, rule, match, **kw):
    with pytest.raises(ValueError, match=match) as e:
        run(**kw)
    assert isinstance(e.value, options.OptionError) and e.value.rule == rule, (kw, e.value)


def test_process_frames_refusals(monkeypatch):
    run = _refusing_process_frames(monkeypatch)
    for bad in ("secam", "", None, "PAL", True, 1):
        _refused(run, "signal_standard", "signal_standard must be", in_signal="composite", signal_standard=bad)
    for bad in ("comb", "", None, "DELAY", 0, True):
        _refused(run, "pal_decoder", "pal_decoder must be", in_signal="composite", signal_standard="pal", pal_decoder=bad)
    for bad in (True, False, 20.0, "20", None, 181, -181, 360):
        for standard in ("ntsc", "pal"):
            _refused(run, "signal_phase", "signal_phase must be an integer", in_signal="composite", signal_standard=standard, signal_phase=bad)
    for kw in (dict(pal_decoder="simple"), dict(signal_phase=20), dict(in_signal="composite", pal_decoder="simple"), dict(in_signal="svideo", signal_phase=-1),
               dict(in_signal="composite", signal_standard="ntsc", pal_decoder="simple", signal_phase=5)):
        _refused(run, "pal_off", "only the PAL decoder has a delay line and a phase knob", **kw)
    for kw in (dict(signal_standard="pal"), dict(signal_standard="pal", in_signal="rgb", pal_decoder="simple", signal_phase=20)):
        _refused(run, "pal_signal", "there is no signal to decode", **kw)
    # the rules in front keep their place
    _refused(run, "signal_off", "no signal to decode", signal_standard="pal", signal_chroma="soft")
    _refused(run, "signal_host", "resize_on='host' cannot be combined with in_signal", in_signal="composite", signal_standard="pal", resize_on="host")
    _refused(run, "in_chroma_rows_format", "only a 4:2:0 input", in_signal="composite", signal_standard="pal", in_chroma_rows="interlaced")
    # what is admitted: the next thing asked for is the device
    for kw in (dict(in_signal="composite", signal_standard="pal"), dict(in_signal="svideo", signal_standard="pal", pal_decoder="simple", signal_phase=-180),
               dict(in_signal="composite", signal_standard="pal", signal_phase=180, signal_chroma="soft", signal_crawl=False),
               dict(in_signal="composite", signal_standard="pal", in_pix_fmt="yuv420p", in_chroma_rows="interlaced", deinterlace="edge", deinterlace_fields="both"),
               dict(in_signal="composite", signal_standard="pal", chain_pix="half", pal_decoder="simple", signal_phase=20),
               dict(in_signal="composite", signal_standard="ntsc", pal_decoder="delay", signal_phase=0), dict(signal_standard="ntsc"), dict()):
        with pytest.raises(AssertionError, match="the device was asked for"):
            run(**kw)
    import pythoncrt_amd as pc
    doc = " ".join(pc.process_frames.__doc__.split())
    for text in ('`signal_standard="pal"`', "270 degrees per line", "Hanover bars", "no 25 Hz offset", "no RF noise", "consecutive lines", "NTSC has no phase knob"):
        assert text in doc, text


def test_cli_refusals_and_the_sharded_cli(tmp_path, monkeypatch):
    from pythoncrt_amd import cli
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("CRTFX_FORCE_DIST", raising=False)
    src = tmp_path / "in.rgb"
    src.write_bytes(bytes(48 * 80 * 3))
    out = tmp_path / "out.rgb"
    base = ["--input", str(src), "--output", str(out), "--width", "80", "--height", "48"]

    def refused(extra, rule, *words):
        with pytest.raises(SystemExit) as e:
            cli.main(base + extra)
        assert e.value.code not in (0, None) and all(w in str(e.value) for w in words), (extra, str(e.value))
        assert (rule is None and e.value.__cause__ is None) or e.value.__cause__.rule == rule, (extra, e.value.__cause__)
        assert not out.exists()
    refused(["--pal-decoder", "simple"], "pal_off", "--pal-decoder simple", "without --signal-standard pal")
    refused(["--in-signal", "composite", "--signal-phase", "20"], "pal_off", "--signal-phase 20", "only the PAL decoder")
    refused(["--signal-standard", "pal"], "pal_signal", "--signal-standard pal without --in-signal", "no signal to decode")
    for bad in ("181", "-181", "720"):
        refused(["--in-signal", "composite", "--signal-standard", "pal", "--signal-phase", bad], "signal_phase", f"--signal-phase {bad}", "-180..180")
    for extra in (["--signal-standard", "secam"], ["--pal-decoder", "comb"], ["--signal-phase", "20.5"], ["--signal-phase", "x"], ["--signal-standard"],
                  ["--pal-decoder"], ["--signal-phase"]):
        with pytest.raises(SystemExit):                                         # argparse's own refusal
            cli.main(base + ["--in-signal", "composite"] + extra)
    dests = ("signal_standard", "pal_decoder", "signal_phase")
    assert not any(act.dest in dests for act in cli.build_parser()._actions)
    assert not any(act.dest in dests for act in cli.add_output_flags(cli.build_parser())._actions)
    assert sum(act.dest in dests for act in cli.add_input_flags(cli.build_parser())._actions) == 3
    parse = cli.add_input_flags(cli.add_output_flags(cli.build_parser())).parse_args
    a = parse(base)
    spec, ranks = cli.check_flags(a)
    assert (a.signal_standard, a.pal_decoder, a.signal_phase) == ("ntsc", "delay", 0) and spec.signal is None and spec.pal is None
    assert type(spec) is options.ChainOptions and ranks is None
    spec, _ = cli.check_flags(parse(base + ["--in-signal", "composite"]))
    assert type(spec) is options.ChainOptions and spec.signal == ("composite", "sharp", True) and spec.pal is None
    spec, _ = cli.check_flags(parse(base + ["--in-signal", "svideo", "--signal-standard", "pal", "--pal-decoder", "simple", "--signal-phase", "-20", "--signal-chroma", "soft"]))
    assert type(spec) is options.PalChainOptions and spec.signal == ("svideo", "soft", True) and spec.pal == ("simple", -20)
    spec, _ = cli.check_flags(parse(base + ["--in-signal", "composite", "--signal-standard", "pal", "--in-pix-fmt", "yuv420p", "--in-chroma-rows", "interlaced"]))
    assert type(spec) is options.PalFieldChainOptions and spec.pal == ("delay", 0) and spec.in_chroma_rows == "interlaced" and len(spec.signal) == 3
    doc = " ".join(cli.__doc__.split())
    for text in ("--signal-standard pal", "--pal-decoder delay", "--signal-phase DEGREES", "Hanover bars", "no 25 Hz offset, no RF noise", "NTSC has no phase knob"):
        assert text in doc, text
    monkeypatch.setenv("CRTFX_FORCE_DIST", "1")
    for extra in (["--in-signal", "composite", "--signal-standard", "pal"], ["--in-signal", "svideo", "--signal-standard", "pal", "--signal-phase", "20"]):
        refused(extra, None, "--in-signal / --signal-chroma / --signal-crawl is not supported by the sharded CLI")
    refused(["--signal-standard", "pal"], "pal_signal", "no signal to decode")
    refused(["--pal-decoder", "simple"], "pal_off", "without --signal-standard pal")


_RAW = ("resize_on", "out_pix_fmt", "out_matrix", "out_range", "in_pix_fmt", "in_matrix", "in_range", "in_size", "in_chroma", "out_chroma",
        "deliver_size", "in_filter", "deliver_filter", "in_crop", "deliver_fit", "deliver_pad_color", "chain_pix", "dither", "deinterlace",
        "field_order", "deinterlace_fields", "in_lut", "deliver_lut", "deliver_interlace", "deliver_lowpass", "in_signal", "signal_chroma",
        "signal_crawl", "in_chroma_rows", "out_chroma_rows", "signal_standard", "pal_decoder", "signal_phase")


def _defaults():
    import inspect
    import pythoncrt_amd as pc
    sig = inspect.signature(pc.process_frames).parameters
    return {n: sig[n].default for n in _RAW}


def test_pal_rules_fire_on_the_surfaces_they_speak_on():
    """PAL_RULES is a table of its own behind RULES, FIELD_RULES and OUT_FIELD_RULES, which stay as they were: five entries, all in front of
    the sharded branch; the two membership checks speak to the keywords only (argparse has them on the command line)."""
    defaults = _defaults()
    assert (defaults["signal_standard"], defaults["pal_decoder"], defaults["signal_phase"]) == ("ntsc", "delay", 0)
    assert [r.name for r in options.PAL_RULES] == ["signal_standard", "pal_decoder", "signal_phase", "pal_off", "pal_signal"]
    assert all(type(r) is options.Rule and r.early for r in options.PAL_RULES)
    assert [(r.keywords is not None, r.flags is not None) for r in options.PAL_RULES] == [(True, False), (True, False), (True, True), (True, True), (True, True)]
    assert [r.name for r in options.FIELD_RULES] == ["in_chroma_rows", "in_chroma_rows_format", "in_chroma_rows_height"]
    assert [r.name for r in options.OUT_FIELD_RULES] == ["out_chroma_rows", "out_chroma_rows_format", "out_chroma_rows_height"]
    assert len(options.RULES) == 41 and not any("pal" in r.name or r.name in ("signal_standard", "signal_phase") for r in options.RULES)
    names = [r.name for r in options.RULES + options.FIELD_RULES + options.OUT_FIELD_RULES + options.PAL_RULES]
    assert len(set(names)) == len(names)

    def raw(hw=(36, 64), **kw):
        return options.Raw(render_hw=hw, **{n: kw.get(n, d) for n, d in defaults.items()})
    fired = set()
    cases = [("signal_standard", dict(signal_standard="secam"), ("keywords",)), ("pal_decoder", dict(pal_decoder="comb"), ("keywords",)),
             ("signal_phase", dict(signal_phase=181), ("keywords", "flags")), ("pal_off", dict(signal_phase=20), ("keywords", "flags")),
             ("pal_off", dict(in_signal="composite", pal_decoder="simple"), ("keywords", "flags")),
             ("pal_signal", dict(signal_standard="pal"), ("keywords", "flags")),
             ("pal_signal", dict(signal_standard="pal", in_signal="composite", pal_decoder="simple", signal_phase=-180), ())]
    for name, kw, surfaces in cases:
        for surface in ("keywords", "flags"):
            for early in (None, True):
                try:
                    options.refuse(raw(**kw), surface, early)
                    got = None
                except options.OptionError as e:
                    got = e.rule
                if surface in surfaces:
                    assert got == name, (name, kw, surface, early, got)
                else:
                    assert got not in [r.name for r in options.PAL_RULES][:[r.name for r in options.PAL_RULES].index(name) + 1], (name, kw, surface, got)
            options.refuse(raw(**{k: v for k, v in kw.items()}), surface, False)                  # behind the branch none of the five is walked
            fired |= {(name, surface)} if surface in surfaces else set()
    assert fired == {(r.name, s) for r in options.PAL_RULES for s in ("keywords", "flags") if getattr(r, s) is not None}
    # class-level defaults: a Raw and a spec built without the three values are what they were
    bare = options.Raw(render_hw=(8, 8))
    assert (bare.signal_standard, bare.pal_decoder, bare.signal_phase) == ("ntsc", "delay", 0)
    for cls in (options.ChainOptions, options.FieldChainOptions):
        assert (cls.signal_standard, cls.pal_decoder, cls.signal_phase) == ("ntsc", "delay", 0)
        assert not {"signal_standard", "pal_decoder", "signal_phase"} & set(cls.__dataclass_fields__)
    assert list(options.FieldChainOptions.__dataclass_fields__)[-2:] == ["in_chroma_rows", "out_chroma_rows"]
    for cls, base in ((options.PalChainOptions, options.ChainOptions), (options.PalFieldChainOptions, options.FieldChainOptions)):
        assert issubclass(cls, base) and list(cls.__dataclass_fields__)[-3:] == ["signal_standard", "pal_decoder", "signal_phase"]
        assert list(cls.__dataclass_fields__)[:-3] == list(base.__dataclass_fields__)
    old = {n: d for n, d in defaults.items() if n not in ("signal_standard", "pal_decoder", "signal_phase")}
    a = options.ChainOptions.build(options.Raw(render_hw=(8, 10), **old), "keywords")
    b = options.ChainOptions.build(raw(hw=(8, 10)), "keywords")
    assert type(a) is type(b) is options.ChainOptions and a == b and a.pal is None
    c = options.ChainOptions.build(raw(hw=(8, 10), in_signal="composite", signal_standard="pal", signal_phase=20), "keywords")
    assert type(c) is options.PalChainOptions and c.pal == ("delay", 20) and c.signal == ("composite", "sharp", True) and c != b and not c.direct
    d = options.ChainOptions.build(raw(hw=(8, 10), in_signal="composite", signal_standard="pal", in_pix_fmt="nv12", in_chroma_rows="interlaced",
                                       out_pix_fmt="nv12", out_chroma_rows="interlaced"), "keywords")
    assert type(d) is options.PalFieldChainOptions and (d.in_chroma_rows, d.out_chroma_rows, d.pal) == ("interlaced", "interlaced", ("delay", 0))


# ---- which stages SourceEnd builds ----------------------------------------------------------------------------------------------------------------

RESIZES = (ingest.IngestResize, resize16.ResizeHalf, resample.Resample)


@pytest.fixture
def built(monkeypatch):
    """PalSignal, Signal, the deinterlacers, Canvas, the resize plans, Widen and Lut3D record (class, positional arguments, keywords) instead of creating a plan."""
    log = []
    for cls in RESIZES + (pal_mod.PalSignal, signal_mod.Signal, deint.Deinterlace, adeint.AdaptiveDeinterlace, canvas.Canvas, depth.Widen, lut3d.Lut3D):
        def init(self, *args, _cls=cls, **kw):
            log.append((_cls, args, kw))
        monkeypatch.setattr(cls, "__init__", init)
    return log


class _Plan:
    frame_bytes = 777


def _source_end(monkeypatch, fmt="rgb24", src_hw=(24, 32), render=(24, 32), **kw):
    monkeypatch.setattr(formats, "source_plan", lambda *a: None if a[2] == "rgb24" else _Plan())
    return ends.SourceEnd("dev", render, fmt, "bt601", "tv", "replicate", src_hw, kw.pop("in_filter", "bilinear"), **kw)


def test_source_end_stages(built, monkeypatch):
    import torch
    u8, f16 = torch.uint8, torch.float16
    R, S = (24, 32), (48, 72)
    # "ntsc": without the keyword, and with None, a Signal with today's keywords and no PalSignal
    for kw in (dict(), dict(pal=None)):
        del built[:]
        end = _source_end(monkeypatch, dtype=u8, signal=("composite", "soft", True), **kw)
        assert built == [(signal_mod.Signal, ("dev", R), {"signal": "composite", "chroma": "soft", "crawl": True, "dtype": u8})]
        assert type(end.signal) is signal_mod.Signal
        del built[:]
        end = _source_end(monkeypatch, **kw)
        assert built == [] and end.stages == [] and end.signal is None and end.index == 0
    # no signal, no PalSignal: the keyword alone builds nothing
    del built[:]
    end = _source_end(monkeypatch, pal=("simple", 20))
    assert built == [] and end.signal is None
    # "pal": a PalSignal in the Signal's place, at the source's size and on the stages' pixel type
    for pix, cable, pal in ((u8, ("composite", "sharp", True), ("delay", 0)), (f16, ("svideo", "soft", False), ("simple", -20))):
        del built[:]
        end = _source_end(monkeypatch, dtype=pix, signal=cable, pal=pal)
        assert built == [(pal_mod.PalSignal, ("dev", R), {"signal": cable[0], "chroma": cable[1], "crawl": cable[2], "decoder": pal[0], "phase": pal[1],
                                                        "dtype": pix})]
        assert [hw for _, hw in end.stages] == [R] and end.stages[0][0] is end.signal and type(end.signal) is pal_mod.PalSignal and end.ratio == 1
    del built[:]
    end = _source_end(monkeypatch, "nv12", S, crop=(2, 4, 40, 60), widen=True, dtype=f16, deinterlace=("adaptive", "bff", "both"), lut="cube",
                      signal=("composite", "soft", True), pal=("delay", 15), chroma_rows="interlaced")
    assert [b[0] for b in built] == [pal_mod.PalSignal, adeint.AdaptiveDeinterlace, canvas.Canvas, ingest.IngestResize, depth.Widen, lut3d.Lut3D]
    assert built[0] == (pal_mod.PalSignal, ("dev", S), {"signal": "composite", "chroma": "soft", "crawl": True, "decoder": "delay", "phase": 15, "dtype": u8})
    assert [hw for _, hw in end.stages] == [S, S, S, (40, 60), R, R, R] and end.ratio == 2
    # convert() hands the PalSignal the index, as it hands it to the Signal
    calls = []
    end = _source_end(monkeypatch, "nv12", S, signal=("composite", "sharp", True), pal=("delay", 0))
    monkeypatch.setattr(torch, "empty", lambda shape, dtype=None, device=None, _e=torch.empty: _e(shape, dtype=dtype))
    end.slots(2, 2, pinned=False)
    for st, _ in end.stages:
        st.run = lambda x, out, _st=st, **kw: calls.append((type(_st), kw)) or out
    end.index = 7
    end.convert(0, 2, torch.zeros((2,) + R + (3,), dtype=u8))
    assert calls == [(_Plan, {}), (pal_mod.PalSignal, {"index": 7}), (ingest.IngestResize, {})]


def test_the_spec_passes_the_keyword_only_for_pal(monkeypatch):
    import torch
    sources = []
    monkeypatch.setattr(ends, "SourceEnd", lambda *a, **kw: sources.append((a, kw)))
    defaults = _defaults()

    def spec(**kw):
        return options.ChainOptions.build(options.Raw(render_hw=(8, 10), **{n: kw.get(n, d) for n, d in defaults.items()}), "keywords")
    spec(in_signal="composite").source_end("dev", (8, 10), torch.uint8)
    spec(in_signal="composite", signal_standard="pal", pal_decoder="simple", signal_phase=20).source_end("dev", (8, 10), torch.uint8)
    spec(in_signal="svideo", signal_standard="pal", in_pix_fmt="nv12", in_chroma_rows="interlaced").source_end("dev", (8, 10), torch.uint8)
    assert "pal" not in sources[0][1] and sources[0][1]["signal"] == ("composite", "sharp", True)
    assert sources[1][1]["pal"] == ("simple", 20) and sources[1][1]["signal"] == ("composite", "sharp", True)
    assert {k: v for k, v in sources[1][1].items() if k != "pal"} == sources[0][1] and sources[1][0] == sources[0][0]
    assert sources[2][1]["pal"] == ("delay", 0) and sources[2][1]["chroma_rows"] == "interlaced" and sources[2][1]["signal"] == ("svideo", "sharp", True)
