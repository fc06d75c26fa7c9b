"""Integer numpy model of the composite-video stage, written from include/crtfx_signal.h: uint8 and half frames, both signals, both decoder
chroma filters, crawl on and off, any frame index.  Everything is int64 and every >> a floor.  The quantiser, the code conversions, `bits`
and `noise` are those of tests/deint_model.py (one quantiser in the library, one in the models)."""
import numpy as np

from tests.deint_model import QMAX, bits, codes, from_codes, noise, quantise  # noqa: F401 - re-exported

SIGNALS = ("composite", "svideo")
CHROMAS = ("sharp", "soft")
COS = np.array([1, 0, -1, 0], dtype=np.int64)
SIN = np.array([0, 1, 0, -1], dtype=np.int64)
T7 = np.array([1, 2, 3, 4, 3, 2, 1], dtype=np.int64)                            # sums to 16
T15 = np.array([1, 2, 3, 4, 5, 6, 7, 8, 7, 6, 5, 4, 3, 2, 1], dtype=np.int64)   # sums to 64
DECODER = {"sharp": (T7, 4), "soft": (T15, 6)}
TO_YIQ = np.array([[1225, 2404, 467], [2441, -1125, -1316], [866, -2141, 1275]], dtype=np.int64)          # 16 per code, >> 8
TO_RGB = np.array([[4096, 3916, 2543], [4096, -1114, -2651], [4096, -4533, 6981]], dtype=np.int64)        # >> 16
ENC_REACH, NOTCH_REACH = 3, 2
HALO = {"sharp": 8, "soft": 12}         # 3 + 2 + the decoder filter's reach
ACC_MAX = int(9.3e8)                    # the last accumulator, by the sum of absolute values, as the header states it


def top(dtype):
    """M: the largest code of a sample type."""
    return 255 if np.dtype(dtype) == np.uint8 else QMAX


def _fir(v, taps, shift):
    """(sum_k taps[k] v(x + k - r) + half) >> shift over the last axis; the result is 2 r shorter."""
    n = v.shape[-1] - len(taps) + 1
    acc = np.full(v.shape[:-1] + (n,), 1 << (shift - 1), dtype=v.dtype)
    for k, t in enumerate(taps):
        acc += v.dtype.type(t) * v[..., k:k + n]
    return acc, acc >> shift


def cascade(c, signal="composite", chroma="sharp", crawl=True, index=0, acc=None):
    """The codes [n, h, w, 3] of n consecutive frames, the first of them frame `index` of the stream -> the unclamped R, G, B (the caller
    clamps them to 0..M, M = `top`); `acc`, a list, receives the largest |final accumulator|.  The arithmetic runs in the integer type
    of `c`: int64 as `codes` gives it, or int32, which the header's bounds allow and a sweep of 2^24 colours needs."""
    assert signal in SIGNALS and chroma in CHROMAS and c.ndim == 4 and c.shape[-1] == 3 and c.dtype in (np.int64, np.int32)
    n, h, w, _ = c.shape
    taps, shift = DECODER[chroma]
    r = len(taps) // 2
    halo = ENC_REACH + NOTCH_REACH + r
    xs = np.arange(-halo, w + halo)                                              # the extended row: the edge pixels replicated
    ext = c[:, :, np.clip(xs, 0, w - 1), :]
    it = c.dtype.type
    y0, i0, q0 = ((it(m[0]) * ext[..., 0] + it(m[1]) * ext[..., 1] + it(m[2]) * ext[..., 2] + it(128)) >> 8 for m in TO_YIQ)
    _, i1 = _fir(i0, T7, 4)
    _, q1 = _fir(q0, T7, 4)
    x1 = xs[ENC_REACH:len(xs) - ENC_REACH]
    t = index + np.arange(n)

    def phase(x):
        return (x[None, None, :] + 2 * np.arange(h)[None, :, None] + (2 * t[:, None, None] if crawl else 0)) % 4     # non-negative

    cos, sin = COS.astype(c.dtype), SIN.astype(c.dtype)
    ch = i1 * cos[phase(x1)] + q1 * sin[phase(x1)]
    y1 = y0[..., ENC_REACH:y0.shape[-1] - ENC_REACH]
    if signal == "composite":
        s = y1 + ch
        assert s.size == 0 or (s.min() >= -32768 and s.max() <= 32767)
        yd = (s[..., :-4] + 2 * s[..., 2:-2] + s[..., 4:] + 2) >> 2
        e = s[..., 2:-2] - yd
    else:
        yd, e = y1[..., 2:-2], ch[..., 2:-2]
    x2 = x1[NOTCH_REACH:len(x1) - NOTCH_REACH]
    _, idm = _fir(2 * e * cos[phase(x2)], taps, shift)
    _, qdm = _fir(2 * e * sin[phase(x2)], taps, shift)
    ydm = yd[..., r:yd.shape[-1] - r]
    assert ydm.shape[-1] == w
    rgb = np.stack([it(m[0]) * ydm + it(m[1]) * idm + it(m[2]) * qdm + it(32768) for m in TO_RGB], axis=-1)
    if acc is not None and rgb.size:
        acc.append(int(np.abs(rgb).max()))
    assert rgb.size == 0 or np.abs(rgb).max() <= ACC_MAX
    return rgb >> 16


def signal(frames, signal="composite", chroma="sharp", crawl=True, index=0):   # noqa: A001 - the stage's name
    """frames [n, h, w, 3] uint8 or float16 -> the same shape and dtype: frame i is frame index + i of the stream."""
    frames = np.asarray(frames)
    assert frames.ndim == 4 and index >= 0
    out = np.zeros(frames.shape, frames.dtype)
    n = frames.shape[0]
    step = max(1, (1 << 19) // max(1, int(np.prod(frames.shape[1:]))))           # frames per pass: the int64 temporaries stay small
    for j in range(0, n, step):
        v = cascade(codes(frames[j:j + step]), signal, chroma, crawl, index + j)
        out[j:j + step] = from_codes(np.clip(v, 0, top(frames.dtype)), frames.dtype.type)
    return out
