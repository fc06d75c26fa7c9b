"""The composite-video stage without a GPU (include/crtfx_signal.h): the model against a per-pixel restatement of the header and against a
float64 cascade without the intermediate roundings, its properties (flat colours and greys survive, the period-4 stripe turns to colour,
dot crawl, the row and frame periods, the clamps, translation by the carrier's period, the int16 / int32 bounds, the half quantiser, the
smallest sizes), the C-ABI bound symbol for symbol and refusing bad arguments before it touches a device, every refusal of
process_frames(in_signal=) and of the CLI's flags, the stages and buffers of SourceEnd with and without the keyword, and the builds'
registers and LDS against the header."""
import ctypes
import itertools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pythoncrt_amd import _lib, _stage, adeint, canvas, deint, depth, ends, formats, ingest, lut3d, resample, resize16  # noqa: E402
from pythoncrt_amd import signal as signal_mod  # noqa: E402
from tests import signal_model as model  # noqa: E402

HEADER = os.path.join(ROOT, "include", "crtfx_signal.h")
DTYPES = (np.uint8, np.float16)
COMBOS = list(itertools.product(model.SIGNALS, model.CHROMAS))


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


def _per_pixel(frames, signal, chroma, crawl, index):
    """The header, one sample at a time: every quantity a function of x on the extended row."""
    n, h, w, _ = frames.shape
    half = frames.dtype == np.float16
    top = 1020 if half else 255
    out = np.zeros(frames.shape, dtype=frames.dtype)
    D, shift = (([1, 2, 3, 4, 3, 2, 1], 4) if chroma == "sharp" else (list(range(1, 9)) + list(range(7, 0, -1)), 6))
    r = len(D) // 2
    T7 = [1, 2, 3, 4, 3, 2, 1]
    for f in range(n):
        t = index + f
        for y in range(h):
            memo = {}

            def ph(x):
                return (x + 2 * y + 2 * (1 if crawl else 0) * t) % 4             # Python's % is non-negative

            def yiq(x):
                if x not in memo:
                    R, G, B = (_code(frames[f, y, min(max(x, 0), w - 1), k]) for k in range(3))
                    memo[x] = ((1225 * R + 2404 * G + 467 * B + 128) >> 8, (2441 * R - 1125 * G - 1316 * B + 128) >> 8,
                               (866 * R - 2141 * G + 1275 * B + 128) >> 8)
                return memo[x]

            def C(x):
                i1 = (sum(T7[k + 3] * yiq(x + k)[1] for k in range(-3, 4)) + 8) >> 4
                q1 = (sum(T7[k + 3] * yiq(x + k)[2] for k in range(-3, 4)) + 8) >> 4
                return i1 * COS[ph(x)] + q1 * SIN[ph(x)]

            def s(x):
                return yiq(x)[0] + C(x)

            def Yd(x):
                return (s(x - 2) + 2 * s(x) + s(x + 2) + 2) >> 2 if signal == "composite" else yiq(x)[0]

            def e(x):
                return s(x) - Yd(x) if signal == "composite" else C(x)
            for x in range(w):
                Id = (sum(D[k + r] * 2 * e(x + k) * COS[ph(x + k)] for k in range(-r, r + 1)) + (1 << (shift - 1))) >> shift
                Qd = (sum(D[k + r] * 2 * e(x + k) * SIN[ph(x + k)] for k in range(-r, r + 1)) + (1 << (shift - 1))) >> shift
                yd = Yd(x)
                rgb = ((4096 * yd + 3916 * Id + 2543 * Qd + 32768) >> 16, (4096 * yd - 1114 * Id - 2651 * Qd + 32768) >> 16,
                       (4096 * yd - 4533 * Id + 6981 * Qd + 32768) >> 16)
                for k in range(3):
                    v = min(max(rgb[k], 0), top)
                    out[f, y, x, k] = np.float16(v / 4.0) if half else v
    return out


def test_names_are_one_list_in_the_model_and_the_module():
    assert signal_mod.SIGNALS == model.SIGNALS == ("composite", "svideo") and signal_mod.CHROMAS == model.CHROMAS == ("sharp", "soft")
    assert signal_mod.Signal.frames_in == 1 and signal_mod.Signal.frames_out == 1
    assert model.T7.sum() == 16 and model.T15.sum() == 64 and model.HALO == {"sharp": 8, "soft": 12}
    assert list(model.COS) == list(COS) and list(model.SIN) == list(SIN)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("signal,chroma", COMBOS)
def test_model_against_the_header_per_pixel(dtype, signal, chroma):
    """Widths from 1 (every tap is the edge pixel) past both halos, heights 1 and 2, crawl on and off, even and odd frame indices."""
    for (h, w), n, crawl, index in (((1, 1), 2, True, 0), ((2, 2), 1, False, 3), ((1, 3), 2, True, 1), ((2, 5), 2, True, 4), ((2, 5), 2, False, 1),
                                    ((3, 27), 1, True, 1)):
        src = _source(dtype, (n, h, w, 3), [h, w, n])
        got = model.signal(src, signal, chroma, crawl, index)
        assert got.dtype == dtype and got.shape == src.shape
        assert np.array_equal(model.bits(got), model.bits(_per_pixel(src, signal, chroma, crawl, index))), (h, w, n, crawl, index)
    ext = _extremes(dtype, (1, 2, 9, 3), 5)
    assert np.array_equal(model.bits(model.signal(ext, signal, chroma, True, 1)), model.bits(_per_pixel(ext, signal, chroma, True, 1)))
    assert model.signal(src[:0], signal, chroma).shape == (0, 3, 27, 3)


def _float_cascade(c, signal, chroma, crawl, index):
    """The cascade on float64 codes with none of the four intermediate roundings (matrix, encoder low-pass, notch, decoder low-pass): the
    three unrounded results per pixel, on the scale of the codes."""
    n, h, w, _ = c.shape
    taps, shift = model.DECODER[chroma]
    r = len(taps) // 2
    halo = 5 + r
    xs = np.arange(-halo, w + halo)
    ext = c[:, :, np.clip(xs, 0, w - 1), :].astype(np.float64)
    yiq = np.einsum("kc,nhxc->knhx", model.TO_YIQ.astype(np.float64), ext) / 256.0

    def fir(v, tp):
        m = v.shape[-1] - len(tp) + 1
        return sum(float(tk) * v[..., k:k + m] for k, tk in enumerate(tp)) / float(sum(tp))

    def phase(x):
        return (x[None, None, :] + 2 * np.arange(h)[None, :, None] + (2 * (index + np.arange(n))[:, None, None] if crawl else 0)) % 4
    x1 = xs[3:-3]
    ch = fir(yiq[1], model.T7) * model.COS[phase(x1)] + fir(yiq[2], model.T7) * model.SIN[phase(x1)]
    y1 = yiq[0][..., 3:-3]
    if signal == "composite":
        s = y1 + ch
        yd = (s[..., :-4] + 2 * s[..., 2:-2] + s[..., 4:]) / 4.0
        e = s[..., 2:-2] - yd
    else:
        yd, e = y1[..., 2:-2], ch[..., 2:-2]
    x2 = x1[2:-2]
    idm, qdm = fir(2 * e * model.COS[phase(x2)], taps), fir(2 * e * model.SIN[phase(x2)], taps)
    return np.einsum("kc,cnhx->nhxk", model.TO_RGB.astype(np.float64), np.stack([yd[..., r:yd.shape[-1] - r], idm, qdm])) / 65536.0


def _float_bound(signal):
    """Each rounding's half unit, carried through the gains behind it, on the 16-per-code scale of Y / I / Q.
    The matrix: 1/2 on each of Y0, I0, Q0.  T7 has gain 1 and rounds: I1, Q1 and with them C are off by at most 1/2 + 1/2 = 1.
    composite: s = Y0 + C by 3/2; Yd, a mean of gain 1 that rounds, by 3/2 + 1/2 = 2; e = s - Yd is (-ds(x - 2) + 2 ds(x) - ds(x + 2)) / 4
    minus the notch's own rounding: 3/2 + 1/2 = 2.  svideo: Yd = Y0 by 1/2, e = C by 1.
    The demodulated products 2 e cos are off by twice that at every other sample and exact (zero) between; the taps of T7 and T15 at every
    other sample sum to half the filter (8 / 16, 32 / 64), so the decoder's filter has gain 1/2 on that error and rounds: Id, Qd by
    eps_c = 2 eps_e / 2 + 1/2 = 5/2 (composite) or 3/2 (svideo).  The last matrix carries those and rounds once more; the clamp is a contraction:
    |out - clip(float)| <= 1/2 + (4096 eps_y + |a| eps_c + |b| eps_c) / 65536 per channel — 0.871 / 0.769 / 1.064 codes (composite) and
    0.679 / 0.617 / 0.795 (svideo)."""
    eps_y, eps_c = (2.0, 2.5) if signal == "composite" else (0.5, 1.5)
    return 0.5 + (np.abs(model.TO_RGB) @ np.array([eps_y, eps_c, eps_c])) / 65536.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("signal,chroma", COMBOS)
def test_model_against_a_float64_cascade_without_the_roundings(dtype, signal, chroma):
    """The integer cascade stays within _float_bound (see its docstring) of the unrounded one, per channel, on noise and on {0, M} noise."""
    bound = _float_bound(signal)
    assert np.allclose(bound, [0.8714, 0.7686, 1.0642] if signal == "composite" else [0.6788, 0.6174, 0.7948], atol=1e-3)
    worst = np.zeros(3)
    for src in (_source(dtype, (2, 5, 41, 3), 7), _extremes(dtype, (2, 4, 33, 3), 8)):
        c = model.codes(src)
        got = model.codes(model.signal(src, signal, chroma, True, 1))
        ref = np.clip(_float_cascade(c, signal, chroma, True, 1), 0, model.top(dtype))
        worst = np.maximum(worst, np.abs(got - ref).reshape(-1, 3).max(axis=0))
    print(f"{signal} {chroma} {np.dtype(dtype).name}: max |integer - float| per channel {worst}, bound {bound}")
    assert (worst <= bound + 1e-9).all(), (worst, bound)


def _flat_is_exact(cols, combos=COMBOS):
    """Every colour of cols [m, 3] as a flat 1 x 4 row: all four sample phases, which are also the phases of every other row and frame
    (on a flat colour a result depends on its phase alone).  In int32, which the header's bounds allow."""
    c = np.broadcast_to(cols.astype(np.int32)[:, None, None, :], (cols.shape[0], 1, 4, 3))
    return all(np.array_equal(model.cascade(c, signal, chroma, True, 0), c) for signal, chroma in combos)


def test_a_flat_colour_returns_itself_for_every_byte_triple():
    """The 4-periodic carrier is averaged exactly by T7 and T15, and the two matrices undo each other on every byte colour: all 256^3 of
    them, in chunks, under composite / sharp — every step of the cascade — and a seeded 2^20 of them under each of the other three rules
    (on a flat colour the notch returns Y0 and every filter its input, so the four rules hold the same numbers at every step: what is
    swept is the pair of matrices)."""
    g = np.arange(256, dtype=np.int32)
    gb = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    for r0 in range(0, 256, 4):
        cols = np.concatenate([np.concatenate([np.full((gb.shape[0], 1), r, dtype=np.int32), gb], axis=1) for r in range(r0, r0 + 4)])
        assert _flat_is_exact(cols, COMBOS[:1]), r0
    rng = np.random.default_rng(10)
    for _ in range(4):
        assert _flat_is_exact(rng.integers(0, 256, (1 << 18, 3)), COMBOS[1:])


def test_a_flat_colour_returns_itself_for_a_sample_of_quarter_code_triples():
    rng = np.random.default_rng(11)
    for combos in (COMBOS[:1], COMBOS[1:2], COMBOS[2:3], COMBOS[3:]):
        assert _flat_is_exact(rng.integers(0, 1021, (1 << 18, 3)), combos)      # 2^20 triples in all, 2^18 under each rule
    corners = np.array(list(itertools.product((0, 1, 510, 1019, 1020), repeat=3)))
    assert _flat_is_exact(corners)


@pytest.mark.parametrize("dtype", DTYPES)
def test_grey_is_exact_under_svideo_and_the_stripe_is_coloured_under_composite(dtype):
    top = model.top(dtype)
    rng = np.random.default_rng(3)
    grey = np.repeat(rng.integers(0, top + 1, (2, 5, 37, 1)), 3, axis=-1)
    frames = model.from_codes(grey, dtype)
    stripe = np.zeros((1, 4, 64, 3), dtype=np.int64)
    stripe[:, :, (np.arange(64) % 4) < 2, :] = top                              # two pixels on, two off: luma detail AT the subcarrier
    stripe = model.from_codes(stripe, dtype)
    for chroma in model.CHROMAS:
        assert np.array_equal(model.bits(model.signal(frames, "svideo", chroma, True, 1)), model.bits(frames))
        assert np.array_equal(model.bits(model.signal(stripe, "svideo", chroma)), model.bits(stripe))
        out = model.codes(model.signal(stripe, "composite", chroma))
        spread = int((out.max(axis=-1) - out.min(axis=-1)).max())
        print(f"{np.dtype(dtype).name} {chroma}: the stripe's channel spread {spread}")
        assert spread > top // 2 and spread <= (245 if dtype == np.uint8 else 979)
        assert not np.array_equal(model.codes(model.signal(frames, "composite", chroma)), grey)        # rainbows on grey detail


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("chroma", model.CHROMAS)
def test_crawl_and_the_row_and_frame_periods(dtype, chroma):
    """A vertical colour edge in rows of equal content: frames t and t + 1 differ under crawl and are equal without it; t and t + 2 are equal;
    rows y and y + 2 are equal, y and y + 1 differ; under svideo nothing depends on the line or the frame."""
    top = model.top(dtype)
    c = np.zeros((4, 6, 40, 3), dtype=np.int64)
    c[..., :20, :] = (top, top // 8, 0)
    c[..., 20:, :] = (0, top // 2, top)
    src = model.from_codes(c, dtype)
    on = model.codes(model.signal(src, "composite", chroma, True, 0))
    off = model.codes(model.signal(src, "composite", chroma, False, 0))
    assert not np.array_equal(on[0], on[1]) and np.array_equal(on[0], on[2]) and np.array_equal(on[1], on[3])
    assert np.array_equal(off[0], off[1]) and np.array_equal(off[0], on[0]) and np.array_equal(off[0], off[3])
    assert np.array_equal(on[1], model.codes(model.signal(src[:1], "composite", chroma, True, 1))[0])
    assert np.array_equal(model.codes(model.signal(src[:1], "composite", chroma, False, 1))[0], off[0])
    assert np.array_equal(on[1, :-1], on[0, 1:])                                # a frame later is a line later: 180 degrees either way
    for v in (on, off):
        assert np.array_equal(v[:, 0], v[:, 2]) and np.array_equal(v[:, 1], v[:, 3]) and not np.array_equal(v[:, 0], v[:, 1])
    sv = model.codes(model.signal(src, "svideo", chroma, True, 0))
    assert np.array_equal(sv, model.codes(model.signal(src, "svideo", chroma, False, 5)))
    assert (sv == sv[0, 0]).all() and not np.array_equal(sv, c)                 # every row of every frame alike, and the edge has bled


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("signal,chroma", COMBOS)
def test_both_clamps_are_driven_and_the_accumulators_stay_small(dtype, signal, chroma):
    src = _extremes(dtype, (2, 8, 64, 3), 21)
    acc = []
    v = model.cascade(model.codes(src), signal, chroma, True, 0, acc)
    top = model.top(dtype)
    out = model.codes(model.signal(src, signal, chroma, True, 0))
    print(f"{signal} {chroma} {np.dtype(dtype).name}: largest accumulator {acc[0]:.3g}, below 0 {np.mean(v < 0):.4f}, above M {np.mean(v > top):.4f}, "
          f"changed {np.mean(out != model.codes(src)):.3f}")
    assert (v < 0).any() and (v > top).any() and out.min() == 0 and out.max() == top
    assert acc[0] <= model.ACC_MAX and np.mean(out != model.codes(src)) > 0.5


def test_the_int16_and_int32_bounds_by_the_sum_of_absolute_values():
    """On quarter codes, the wider scale.  Y0 within 0 .. 16320; |I0| <= 9726 and |Q0| <= 8531 (a row's positive or negative coefficients
    at 1020); T7 is a mean, so I1 and Q1 are no larger; s = Y0 + C lies within -9726 .. 16320 + 9726; Yd is a mean of s.  e = s - Yd is
    at most the width of s's range; the demodulated product twice that; the decoder's mean over every other tap half of that again; and
    the last accumulator 4096 |Yd| + (|a| + |b|) |Id| + 32768 — all far inside int32, as the header states."""
    m = model.TO_YIQ
    pos, neg = np.where(m > 0, m, 0).sum(axis=1), np.where(m < 0, m, 0).sum(axis=1)
    hi, lo = (pos * 1020 + 128) >> 8, (neg * 1020 + 128) >> 8
    assert list(hi) == [16320, 9726, 8531] and list(lo) == [0, -9726, -8531]
    s_lo, s_hi = int(lo[1]), int(hi[0] + hi[1])
    assert (s_lo, s_hi) == (-9726, 26046) and -32768 <= s_lo and s_hi <= 32767
    e_max = s_hi - s_lo
    c_max = e_max + 1                                                           # 2 e over half of a filter of gain 1, and its rounding
    last = int(4096 * s_hi + np.abs(model.TO_RGB[:, 1:]).sum(axis=1).max() * c_max + 32768)
    assert last <= model.ACC_MAX < 2 ** 31 and 64 * 2 * e_max + 32 < 2 ** 31 and int(np.abs(m).sum(axis=1).max()) * 1020 + 128 < 2 ** 31
    assert last > 5e8                                                           # the header's 9.3e8 is this bound's order, not a loose one


def test_the_half_quantiser_on_every_pattern():
    h = _all_halves()
    q = model.quantise(h)
    assert q.min() == 0 and q.max() == 1020 and np.array_equal(q, np.array([_code(v) for v in h]))
    frames = np.resize(h, (1, 16, 1366, 3))
    assert np.array_equal(np.unique(model.bits(frames)), np.arange(65536))
    for signal, chroma in COMBOS[:2]:
        out = model.signal(frames, signal, chroma)
        assert np.array_equal(model.bits(out), model.bits(model.signal(model.from_codes(model.quantise(frames), np.float16), signal, chroma)))
        assert np.isfinite(out.astype(np.float32)).all() and np.array_equal(model.quantise(out).astype(np.float64) / 4.0, out.astype(np.float64))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("signal,chroma", COMBOS)
def test_a_shift_by_the_carriers_period_commutes_away_from_the_edges(dtype, signal, chroma):
    src = _source(dtype, (2, 3, 72, 3), 31)
    moved = np.roll(src, 4, axis=2)
    a, b = model.signal(src, signal, chroma, True, 1), model.signal(moved, signal, chroma, True, 1)
    halo = model.HALO[chroma]
    assert np.array_equal(model.bits(b[:, :, halo + 4:72 - halo]), model.bits(a[:, :, halo:72 - halo - 4]))
    moved1 = np.roll(src, 1, axis=2)
    if signal == "composite":
        assert not np.array_equal(model.bits(model.signal(moved1, signal, chroma, True, 1)[:, :, halo + 1:72 - halo]), model.bits(a[:, :, halo:72 - halo - 1]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_smallest_sizes(dtype):
    """Widths 1, 2, 3, 5 and heights 1, 2: narrower than every filter, so every tap is an edge pixel; a one-pixel row is a flat colour."""
    for signal, chroma in COMBOS:
        for h, w in itertools.product((1, 2), (1, 2, 3, 5)):
            src = _source(dtype, (3, h, w, 3), [h, w])
            out = model.signal(src, signal, chroma, True, 2)
            assert out.shape == src.shape and out.dtype == dtype
            if w == 1:
                assert np.array_equal(model.codes(out), model.codes(src))
            wide = np.concatenate([np.repeat(src[:, :, :1], 12, axis=2), src, np.repeat(src[:, :, -1:], 12, axis=2)], axis=2)
            assert np.array_equal(model.bits(model.signal(wide, signal, chroma, True, 2)[:, :, 12:12 + w]), model.bits(out))


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------------------

_vp = ctypes.c_void_p
SIGNATURES = {
    "crtfx_signal_create": (ctypes.c_int, [ctypes.c_int] * 7 + [ctypes.POINTER(_vp)]),
    "crtfx_signal_destroy": (ctypes.c_int, [_vp]),
    "crtfx_signal_last_error": (ctypes.c_char_p, [_vp]),
    "crtfx_signal_run": (ctypes.c_int, [_vp, ctypes.c_int64, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_int, _vp]),
    "crtfx_signal_set_option": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "crtfx_signal_last_plan": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_size_t]),
}


def test_symbols_are_bound_and_the_header_declares_them():
    assert _lib.SIGNAL_SYMBOLS == SIGNATURES and list(_lib.SIGNAL_SYMBOLS) == list(SIGNATURES) and _lib.SIGNAL_OPT_FORCE_GENERAL == 1
    assert _lib.SIGNAL_SYMBOLS == _lib.frame_symbols("signal", [ctypes.c_int] * 6, run=SIGNATURES["crtfx_signal_run"])
    assert (_lib.SIGNAL_COMPOSITE, _lib.SIGNAL_SVIDEO, _lib.SIGNAL_SHARP, _lib.SIGNAL_SOFT) == (0, 1, 0, 1)
    lib = _lib.load()
    for name, (res, args) in SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res, name
    hdr = open(HEADER).read()
    for text in ("CRTFX_SIGNAL_OPT_FORCE_GENERAL = 1", "CRTFX_SIGNAL_COMPOSITE = 0", "CRTFX_SIGNAL_SVIDEO = 1", "CRTFX_SIGNAL_SHARP = 0",
                 "CRTFX_SIGNAL_SOFT = 1", "NOT claimed is equality with any other NTSC implementation", "no PAL, no burst-axis rotation, no RF noise",
                 "signal=k_signal<composite,soft,u8,vec>;frames=5", "(1225 R + 2404 G +  467 B + 128) >> 8", "4096 Yd - 4533 Id + 6981 Qd + 32768"):
        assert text in hdr, text
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(crtfx_signal_\w+)\s*\(([^)]*)\)\s*;", hdr)}
    assert set(protos) == set(SIGNATURES) and len(protos) == 6, set(protos) ^ set(SIGNATURES)
    for name, args in protos.items():
        assert len(args.split(",")) == len(SIGNATURES[name][1]), name
    order = [a.split()[-1].lstrip("*") for a in protos["crtfx_signal_create"].split(",")]
    assert order == ["device", "h", "w", "pix_fmt", "signal", "chroma", "crawl", "out_plan"]
    order = [a.split()[-1].lstrip("*") for a in protos["crtfx_signal_run"].split(",")]
    assert order[:2] == ["plan", "first_index"] and "int64_t first_index" in protos["crtfx_signal_run"]
    others = set()
    for table in ("SYMBOLS", "INGEST_SYMBOLS", "EGRESS_SYMBOLS", "UNPACK_SYMBOLS", "DEEP_SYMBOLS", "YUV422_SYMBOLS", "DEEP444_SYMBOLS", "SITED_SYMBOLS",
                  "EGRESS_SITED_SYMBOLS", "RESIZE16_SYMBOLS", "RESAMPLE_SYMBOLS", "CANVAS_SYMBOLS", "DEPTH_SYMBOLS", "DEINT_SYMBOLS", "ADEINT_SYMBOLS",
                  "LUT3D_SYMBOLS", "INTERLACE_SYMBOLS"):
        others |= set(getattr(_lib, table))
    assert not set(SIGNATURES) & others
    assert all(os.path.basename(f) in {os.path.basename(s) for s in _lib.SOURCES} for f in ("crtfx_signal.hip", "crtfx_signal.h", "crtfx_frame_host.h"))
    assert all(os.path.exists(s) for s in _lib.SOURCES) and "crtfx_signal" in _lib.STAGE_UNITS
    import pythoncrt_amd as pc
    assert pc.Signal is signal_mod.Signal and "Signal" in pc.__all__
    assert issubclass(pc.Signal, _stage.FramePlan) and not issubclass(pc.Signal, _stage.StagePlan) and not issubclass(pc.Signal, _stage.ResizePlan)
    assert pc.Signal._family == "signal" and pc.Signal._force_option == 1
    unit = open(os.path.join(_lib.CSRC, "crtfx_signal.hip")).read()
    assert "namespace crtfx_signal_impl" in unit and "crtfx_frames::run<U>" in unit and "hipGetDevice" not in unit        # run() is the skeleton's
    assert "asm" not in unit
    import bench                                                               # a namespace of its own, outside the chain's evidence hash
    assert "crtfx_signal" not in open(bench.__file__).read()


GOOD = dict(device=0, h=9, w=24, pix_fmt=_lib.PIX_U8, signal=_lib.SIGNAL_COMPOSITE, chroma=_lib.SIGNAL_SOFT, crawl=1)


def _create(lib, no_out=False, **kw):
    a = dict(GOOD)
    a.update(kw)
    plan = ctypes.c_void_p(1)
    rc = lib.crtfx_signal_create(*(a[k] for k in GOOD), None if no_out else ctypes.byref(plan))
    return rc, plan, (lib.crtfx_signal_last_error(None) or b"").decode()


def test_create_refuses_bad_arguments_before_it_touches_a_device():
    """Every refusal of crtfx_signal_create comes before the device is asked for, so it holds on any machine; *out_plan is NULL and the
    message names the offending field.  The call that passes every check is left with the device: `no HIP device 4096`."""
    lib = _lib.load()
    cases = [({k: v}, f"{k} = {v} outside 1..32767") for k in ("h", "w") for v in (0, -3, 32768)]
    cases += [({k: v}, f"unknown {k} {v}") for k in ("pix_fmt", "signal", "chroma") for v in (2, -1, 7)]
    cases += [(dict(crawl=v), f"crawl = {v}") for v in (2, -1, 7)]
    for kw, text in cases:
        rc, plan, msg = _create(lib, **kw)
        assert rc == _lib.E_INVALID and not plan.value and text in msg, (kw, rc, plan.value, msg)
    rc, plan, msg = _create(lib, no_out=True)
    assert rc == _lib.E_INVALID and "out_plan" in msg
    for kw in (dict(), dict(h=1, w=1), dict(h=32767, w=32767, pix_fmt=_lib.PIX_F16), dict(signal=1, chroma=0, crawl=0), dict(chroma=0)):
        rc, plan, msg = _create(lib, device=4096, **kw)
        assert rc == _lib.E_HIP and not plan.value and "no HIP device 4096" in msg, (kw, rc, msg)
    assert lib.crtfx_signal_destroy(None) == _lib.OK and lib.crtfx_signal_set_option(None, 1, 1) == _lib.E_INVALID
    assert lib.crtfx_signal_run(None, 0, None, 0, None, 0, 1, None) == _lib.E_INVALID
    assert lib.crtfx_signal_last_plan(None, ctypes.create_string_buffer(8), 8) == _lib.E_INVALID


def test_python_plan_refuses_before_a_device():
    for kw in (dict(signal="rf"), dict(chroma="blurry"), dict(signal=None), dict(chroma=1), dict(crawl=1), dict(crawl="on"), dict(crawl=None)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            signal_mod.Signal("cpu", (4, 4), **kw)
    with pytest.raises(ValueError, match="ROCm device"):
        signal_mod.Signal("cpu", (4, 4))
    plan = signal_mod.Signal.__new__(signal_mod.Signal)
    plan._index = 3
    for bad in (-1, 1.5, None, True):
        with pytest.raises(ValueError, match="index"):
            plan.reset(bad)
    plan.reset(6)
    assert plan._index == 6
    plan.reset()
    assert plan._index == 0
    for text in ("4 x fsc", "SD-width", "behind the stage"):
        assert text in signal_mod.__doc__ and text in " ".join((signal_mod.Signal.__doc__ + " x").split()), text


# what include/crtfx_signal.h states for the sixteen builds: VGPRs as built
HEADER_VGPRS = {
    "k_signal<composite,sharp,u8,vec>": 50, "k_signal<composite,sharp,f16,vec>": 49, "k_signal<composite,soft,u8,vec>": 57,
    "k_signal<composite,soft,f16,vec>": 53, "k_signal<svideo,sharp,u8,vec>": 50, "k_signal<svideo,sharp,f16,vec>": 41,
    "k_signal<svideo,soft,u8,vec>": 56, "k_signal<svideo,soft,f16,vec>": 50, "k_signal<composite,sharp,u8,general>": 59,
    "k_signal<composite,sharp,f16,general>": 59, "k_signal<composite,soft,u8,general>": 83, "k_signal<composite,soft,f16,general>": 83,
    "k_signal<svideo,sharp,u8,general>": 45, "k_signal<svideo,sharp,f16,general>": 45, "k_signal<svideo,soft,u8,general>": 60,
    "k_signal<svideo,soft,f16,general>": 60}
VEC_LDS = 4 * 4 * 528 * 2


def test_signal_kernels_have_no_scratch_and_the_headers_registers_and_lds():
    """Registers, LDS and scratch of the sixteen builds, read from the built library's code objects (tools/kernel_resources.py): no scratch
    memory, no spills, no AGPRs, 16896 bytes of LDS for the vec builds and none for the general ones — and the figures the header quotes
    are the figures of this build."""
    import kernel_resources
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    res = kernel_resources.resources(_lib.LIB_PATH)
    found = {n.replace("crtfx_signal_impl::", "").replace("crtfx_deint_impl::", "").replace(", ", ","): v
             for n, v in res.items() if n.startswith("crtfx_signal_impl::")}
    assert set(found) == set(HEADER_VGPRS), sorted(found)
    hdr = open(HEADER).read()
    for name, v in found.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["group_segment_fixed_size"] == (VEC_LDS if name.endswith(",vec>") else 0) and v["agpr_count"] == 0, (name, v)
        assert v["vgpr_count"] == HEADER_VGPRS[name], (name, v["vgpr_count"])
        assert re.search(rf"{re.escape(name)} {HEADER_VGPRS[name]}\b", hdr), name
    assert f"LDS: {VEC_LDS} bytes per workgroup for every vec build" in hdr and "no AGPRs, no scratch, no spills" in hdr
    assert len([n for n in res if n.startswith("crtfx_deint_impl::")]) == 16    # the deinterlacer's builds are its own still


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
    return lambda h=46, **kw: pc.process_frames(never(), lambda a: None, 80, h, 30.0, 1, **kw)


def test_process_frames_refusals(monkeypatch):
    run = _refusing_process_frames(monkeypatch)
    for bad in ("on", "", None, "COMPOSITE", True, 1, "ntsc", "off"):
        with pytest.raises(ValueError, match="in_signal must be"):
            run(in_signal=bad)
    for bad in ("blurry", "", None, "SOFT", 0):
        for signal in ("rgb", "composite"):
            with pytest.raises(ValueError, match="signal_chroma must be"):
                run(in_signal=signal, signal_chroma=bad)
    for bad in ("on", None, 0, 1, "off"):
        for signal in ("rgb", "svideo"):
            with pytest.raises(ValueError, match="signal_crawl must be"):
                run(in_signal=signal, signal_crawl=bad)
    for kw in (dict(signal_chroma="soft"), dict(signal_crawl=False), dict(in_signal="rgb", signal_chroma="soft", signal_crawl=False)):
        with pytest.raises(ValueError, match="no signal to decode"):
            run(**kw)
    for signal in model.SIGNALS:
        with pytest.raises(ValueError, match="resize_on='host' cannot be combined with in_signal"):
            run(in_signal=signal, resize_on="host")
    # what is admitted: the next thing asked for is the device
    for kw in (dict(in_signal="composite"), dict(in_signal="svideo", signal_chroma="soft", signal_crawl=False), dict(in_signal="rgb"),
               dict(in_signal="rgb", signal_chroma="sharp", signal_crawl=True, resize_on="host"),
               dict(in_signal="composite", in_pix_fmt="uyvy422", in_size=(48, 72), deinterlace="edge", deinterlace_fields="both"),
               dict(in_signal="composite", chain_pix="half", in_pix_fmt="nv12", in_size=(30, 40), in_filter="lanczos"),
               dict(in_signal="svideo", in_pix_fmt="p010le", out_pix_fmt="yuv444p10le", signal_chroma="soft"), dict()):
        with pytest.raises(AssertionError, match="the device was asked for"):
            run(**kw)
    import pythoncrt_amd as pc
    doc = " ".join(pc.process_frames.__doc__.split())
    for text in ("4 x fsc", "SD-width sources", "the resize to the render size is behind the stage"):
        assert text in doc, text


def test_cli_refusals_and_the_sharded_cli(tmp_path, monkeypatch):
    from pythoncrt_amd import cli
    src = tmp_path / "in.rgb"
    src.write_bytes(bytes(46 * 80 * 3))
    out = tmp_path / "out.rgb"
    base = ["--input", str(src), "--output", str(out), "--width", "80", "--height", "46"]

    def refused(extra, *words, args=base):
        with pytest.raises(SystemExit) as e:
            cli.main(args + extra)
        assert e.value.code not in (0, None) and all(w in str(e.value) for w in words), (extra, str(e.value))
        assert not out.exists()
    refused(["--signal-chroma", "soft"], "--signal-chroma soft", "--in-signal", "no signal to decode")
    refused(["--signal-crawl", "off"], "--signal-crawl off", "no signal to decode")
    refused(["--in-signal", "rgb", "--signal-chroma", "soft", "--signal-crawl", "off"], "no signal to decode")
    for extra in (["--in-signal", "ntsc"], ["--signal-chroma", "blurry"], ["--signal-crawl", "yes"], ["--in-signal"], ["--signal-crawl"]):
        with pytest.raises(SystemExit):                                         # argparse's own refusal of an unknown choice
            cli.main(base + extra)
    dests = ("in_signal", "signal_chroma", "signal_crawl")
    assert not any(act.dest in dests for act in cli.build_parser()._actions)
    assert not any(act.dest in dests for act in cli.add_output_flags(cli.build_parser())._actions)
    assert sum(act.dest in dests for act in cli.add_input_flags(cli.build_parser())._actions) == 3
    parse = cli.add_input_flags(cli.add_output_flags(cli.build_parser())).parse_args
    a = parse(base)
    spec, ranks = cli.check_flags(a)
    assert (a.in_signal, a.signal_chroma, a.signal_crawl) == ("rgb", "sharp", "on") and spec.signal is None
    assert spec.deliver is None and spec.half is False and ranks is None
    a = parse(base + ["--in-signal", "composite"])
    spec, ranks = cli.check_flags(a)
    assert spec.signal == ("composite", "sharp", True) and spec.deliver is None and spec.half is False and ranks is None
    a = parse(base + ["--in-signal", "svideo", "--signal-chroma", "soft", "--signal-crawl", "off"])
    spec, ranks = cli.check_flags(a)
    assert spec.signal == ("svideo", "soft", False)
    doc = " ".join(cli.__doc__.split())
    assert "--in-signal composite --signal-chroma soft" in doc and "four times the colour subcarrier" in doc and "SD-width" in doc
    monkeypatch.setenv("CRTFX_FORCE_DIST", "1")
    for extra in (["--in-signal", "composite"], ["--in-signal", "svideo", "--signal-chroma", "soft"], ["--in-signal", "composite", "--signal-crawl", "off"]):
        refused(extra, "--in-signal / --signal-chroma / --signal-crawl is not supported by the sharded CLI")
    refused(["--signal-chroma", "soft"], "no signal to decode")


# ---- which stages SourceEnd builds, and the buffers behind them ------------------------------------------------------------------------------------

RESIZES = (ingest.IngestResize, resize16.ResizeHalf, resample.Resample)


@pytest.fixture
def built(monkeypatch):
    """Signal, the deinterlacers, Canvas, the resize plans, Widen and Lut3D record (class, positional arguments, keywords) instead of creating a plan."""
    log = []
    for cls in RESIZES + (signal_mod.Signal, deint.Deinterlace, adeint.AdaptiveDeinterlace, canvas.Canvas, depth.Widen, lut3d.Lut3D):
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
    # without the keyword, and with None: what was built before
    for kw in (dict(), dict(signal=None)):
        del built[:]
        end = _source_end(monkeypatch, **kw)
        assert built == [] and end.stages == [] and end.signal is None and end.index == 0
        end = _source_end(monkeypatch, "nv12", S, crop=(2, 4, 40, 60), widen=True, dtype=f16, deinterlace=("edge", "tff", "both"), lut="cube", **kw)
        assert [b[0] for b in built] == [deint.Deinterlace, canvas.Canvas, ingest.IngestResize, depth.Widen, lut3d.Lut3D] and end.signal is None
        assert [type(st) for st, _ in end.stages] == [_Plan, deint.Deinterlace, canvas.Canvas, ingest.IngestResize, depth.Widen, lut3d.Lut3D]
    # an rgb24 frame at render size: the Signal is the only stage, at that size and on the chain's pixel type
    for pix, cable in ((u8, ("composite", "sharp", True)), (f16, ("svideo", "soft", False))):
        del built[:]
        end = _source_end(monkeypatch, dtype=pix, signal=cable)
        assert built == [(signal_mod.Signal, ("dev", R), {"signal": cable[0], "chroma": cable[1], "crawl": cable[2], "dtype": pix})]
        assert [hw for _, hw in end.stages] == [R] and end.stages[0][0] is end.signal and end.ratio == 1
    # everything at once: source plan, SIGNAL at the source's size on uint8, Deinterlace, Canvas, resize, Widen, Lut3D
    del built[:]
    end = _source_end(monkeypatch, "nv12", S, crop=(2, 4, 40, 60), widen=True, dtype=f16, deinterlace=("adaptive", "bff", "both"), lut="cube",
                      signal=("composite", "soft", True))
    assert [b[0] for b in built] == [signal_mod.Signal, adeint.AdaptiveDeinterlace, canvas.Canvas, ingest.IngestResize, depth.Widen, lut3d.Lut3D]
    assert built[0] == (signal_mod.Signal, ("dev", S), {"signal": "composite", "chroma": "soft", "crawl": True, "dtype": u8})
    assert [type(st) for st, _ in end.stages] == [_Plan, signal_mod.Signal, adeint.AdaptiveDeinterlace, canvas.Canvas, ingest.IngestResize, depth.Widen,
                                                  lut3d.Lut3D]
    assert [hw for _, hw in end.stages] == [S, S, S, (40, 60), R, R, R] and end.ratio == 2 and end.frame_bytes == 777
    # a 10-bit source: the Signal runs on half frames
    del built[:]
    end = _source_end(monkeypatch, "p010le", dtype=f16, signal=("svideo", "sharp", True))
    assert built == [(signal_mod.Signal, ("dev", R), {"signal": "svideo", "chroma": "sharp", "crawl": True, "dtype": f16})]


def test_source_end_buffers_and_the_index_the_signal_is_given(built, monkeypatch):
    """slots(): the Signal's buffer holds B SOURCE frames at the source's size (it stands in front of the Deinterlace); convert() hands every
    stage the frames of the one in front, and the Signal the `index` the caller set."""
    import torch
    shapes = []
    real_empty = torch.empty

    class _Pinned:
        def __init__(self, t):
            self.t = t

        def pin_memory(self):
            return self.t

    def empty(shape, dtype=None, device=None):
        shapes.append((tuple(shape), dtype, device))
        return real_empty(shape, dtype=dtype)                                   # on the host: the shapes are what is checked
    monkeypatch.setattr(torch, "empty", empty)
    u8 = torch.uint8
    R, S = (24, 32), (48, 72)
    end = _source_end(monkeypatch, "nv12", S, deinterlace=("edge", "tff", "both"), signal=("composite", "sharp", True))
    end.slots(3, 2, pinned=False)
    assert [s for s in shapes if s[2] == "dev"] == ([((3,) + S + (3,), u8, "dev")] * 2 + [((3,) + S + (3,), u8, "dev")] * 2 +
                                                   [((6,) + S + (3,), u8, "dev")] * 2 + [((3, 777), u8, "dev")] * 2)
    calls = []
    for st, _ in end.stages:
        st.run = lambda x, out, _st=st, **kw: calls.append((type(_st), tuple(x.shape), tuple(out.shape), kw)) or out
    dst = real_empty((6,) + R + (3,), dtype=u8)
    for index in (0, 7):
        del calls[:]
        end.index = index
        end.convert(1, 2, dst[:4])
        assert calls == [(_Plan, (2, 777), (2,) + S + (3,), {}), (signal_mod.Signal, (2,) + S + (3,), (2,) + S + (3,), {"index": index}),
                         (deint.Deinterlace, (2,) + S + (3,), (4,) + S + (3,), {}), (ingest.IngestResize, (4,) + S + (3,), (4,) + R + (3,), {})]
    # without the keyword no stage is told an index
    end = _source_end(monkeypatch, "nv12", S)
    end.slots(2, 2, pinned=False)
    for st, _ in end.stages:
        st.run = lambda x, out, _st=st, **kw: calls.append((type(_st), kw)) or out
    del calls[:]
    end.convert(0, 2, dst[:2])
    assert calls == [(_Plan, {}), (ingest.IngestResize, {})]
