"""Integer numpy model of the interlace stage, written from include/crtfx_interlace.h: uint8 and half frames, TFF and BFF, the three
low-pass settings, odd frame counts.  Everything is int64; under "none" rows are moved as bits.  The quantiser, the code conversions, `bits`
and `noise` are those of tests/deint_model.py (one quantiser in the library, one in the models)."""
import numpy as np

from tests.deint_model import QMAX, bits, codes, from_codes, noise, quantise  # noqa: F401 - re-exported

ORDERS = ("tff", "bff")
LOWPASS = ("none", "linear", "complex")
ACC_MIN, ACC_MAX = -2040, 10204     # COMPLEX's accumulator on quarter codes, as the header states them


def top(dtype):
    """M: the largest code of a sample type."""
    return 255 if np.dtype(dtype) == np.uint8 else QMAX


def rows(c, k):
    """r(k) of every row: row clamp(y + k, 0, h - 1) of the same frame; c is [..., h, w, 3].  A new array."""
    h = c.shape[-3]
    return np.take(c, np.clip(np.arange(h) + k, 0, h - 1), axis=-3)


def weave(a, b, order="tff", lowpass="none"):
    """Output frames of the frames a (first field) and b (second field), [..., h, w, 3] each: row y from a where y % 2 is the first field's
    parity, from b elsewhere, and every r(k) of a row from that row's own frame."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and a.ndim >= 3 and a.shape[-3] >= 2 and a.shape[-1] == 3
    assert order in ORDERS and lowpass in LOWPASS
    first = ORDERS.index(order)                                                 # the parity of the rows frame a gives
    if lowpass == "none":
        out = b.copy()
        out[..., first::2, :, :] = a[..., first::2, :, :]
        return out
    ca, cb = codes(a), codes(b)

    def r(k):
        t = rows(cb, k)
        t[..., first::2, :, :] = rows(ca, k)[..., first::2, :, :]
        return t
    if lowpass == "linear":
        out = (r(-1) + 2 * r(0) + r(1) + 2) >> 2
    else:
        acc = -r(-2) + 2 * r(-1) + 6 * r(0) + 2 * r(1) - r(2) + 4
        assert acc.size == 0 or (acc.min() >= ACC_MIN and acc.max() <= ACC_MAX)
        v = np.clip(acc >> 3, 0, top(a.dtype))                                 # >> on int64 is arithmetic: a floor
        out = np.where(r(-1) + r(1) > 2 * r(0), np.maximum(v, r(0)), np.minimum(v, r(0)))
    return from_codes(out, a.dtype.type)


def filtered(frame, lowpass):
    """A frame with every row low-passed inside that frame: the frame woven with itself."""
    return weave(frame, frame, "tff", lowpass)


def interlace(frames, order="tff", lowpass="none"):
    """frames [n, h, w, 3] uint8 or float16 -> [ceil(n / 2), h, w, 3] of the same dtype: output frame j from frames 2 j and min(2 j + 1, n - 1)."""
    frames = np.asarray(frames)
    assert frames.ndim == 4
    n = frames.shape[0]
    n_out = (n + 1) // 2
    out = np.zeros((n_out,) + frames.shape[1:], frames.dtype)
    step = max(1, (1 << 21) // max(1, int(np.prod(frames.shape[1:]))))                         # pairs per pass: the int64 temporaries stay small
    for j in range(0, n_out, step):
        ja = np.arange(j, min(j + step, n_out))
        out[ja] = weave(frames[2 * ja], frames[np.minimum(2 * ja + 1, n - 1)], order, lowpass)
    return out
