"""Integer numpy model of the PAL composite-video stage, written from include/crtfx_pal.h: uint8 and half frames, both signals, both decoder
chroma filters, both decoders, any phase error, crawl on and off, any frame index.  Everything is int64 and every >> a floor.  The FIR and
its taps are those of tests/signal_model.py, the quantiser, the code conversions, `bits` and `noise` those of tests/deint_model.py."""
import numpy as np

from tests.deint_model import QMAX, bits, codes, from_codes, noise, quantise  # noqa: F401 - re-exported
from tests.signal_model import CHROMAS, COS, DECODER, ENC_REACH, HALO, NOTCH_REACH, SIGNALS, SIN, T7, T15, _fir, top  # noqa: F401 - re-exported

DECODERS = ("delay", "simple")
TO_YUV = np.array([[1225, 2404, 467], [-603, -1183, 1786], [2518, -2109, -409]], dtype=np.int64)         # 16 per code, >> 8
TO_RGB = np.array([[4096, 0, 4670], [4096, -1617, -2379], [4096, 8325, 0]], dtype=np.int64)              # over (Yd, U, V), >> 16
ACC_MAX = int(5.4e8)                    # the last accumulator, by the sum of absolute values, as the header states it
ROT_MAX = int(2.2e8)                    # the rotation's accumulators, likewise


def phase_table(degrees):
    """(c_theta, s_theta) = (llrint(4096 cos theta), llrint(4096 sin theta)) in double."""
    assert -180 <= degrees <= 180
    th = float(degrees) * np.pi / 180.0
    return int(np.rint(4096.0 * np.cos(th))), int(np.rint(4096.0 * np.sin(th)))


def partner_rows(h):
    """y' of every row: y - 1, and for row 0 row 1 (row 0 itself where h = 1)."""
    yp = np.arange(h) - 1
    yp[0] = 1 if h > 1 else 0
    return yp


def rows(c, signal="composite", chroma="sharp", crawl=True, index=0, phase=0, acc=None):
    """Steps 1 - 7 on the codes [n, h, w, 3] of n consecutive frames, the first of them frame `index` of the stream -> (Yd, Ur, Vr), each
    [n, h, w] int64; `acc`, a dict, receives the largest |value| of what the header bounds."""
    assert signal in SIGNALS and chroma in CHROMAS and c.ndim == 4 and c.shape[-1] == 3 and c.dtype == np.int64
    n, h, w, _ = c.shape
    taps, shift = DECODER[chroma]
    r = len(taps) // 2
    halo = ENC_REACH + NOTCH_REACH + r
    xs = np.arange(-halo, w + halo)                                              # the extended row: the edge pixels replicated
    ext = c[:, :, np.clip(xs, 0, w - 1), :]
    y0, u0, v0 = ((m[0] * ext[..., 0] + m[1] * ext[..., 1] + m[2] * ext[..., 2] + 128) >> 8 for m in TO_YUV)
    _, u1 = _fir(u0, T7, 4)
    _, v1 = _fir(v0, T7, 4)
    x1 = xs[ENC_REACH:len(xs) - ENC_REACH]
    line = np.arange(h)[None, :, None] + ((index + np.arange(n))[:, None, None] if crawl else 0)     # y + c t
    sw = np.where(line % 2 == 0, 1, -1)                                          # the V switch

    def phase_of(x):
        return (x[None, None, :] + 3 * line) % 4                                 # non-negative

    ch = u1 * SIN[phase_of(x1)] + sw * v1 * COS[phase_of(x1)]
    y1 = y0[..., ENC_REACH:y0.shape[-1] - ENC_REACH]
    if signal == "composite":
        s = y1 + ch
        yd = (s[..., :-4] + 2 * s[..., 2:-2] + s[..., 4:] + 2) >> 2
        e = s[..., 2:-2] - yd
    else:
        s, yd, e = ch, y1[..., 2:-2], ch[..., 2:-2]
    x2 = x1[NOTCH_REACH:len(x1) - NOTCH_REACH]
    _, ud = _fir(2 * e * SIN[phase_of(x2)], taps, shift)
    _, vd = _fir(2 * e * sw * COS[phase_of(x2)], taps, shift)
    ct, st = phase_table(phase)
    au, av = ct * ud + sw * st * vd + 2048, ct * vd - sw * st * ud + 2048
    ydm = yd[..., r:yd.shape[-1] - r]
    assert ydm.shape[-1] == w and ud.shape[-1] == w
    if acc is not None and ud.size:
        for name, val in (("y0", y0), ("u0", u0), ("v0", v0), ("s", s), ("e", e), ("ud", np.maximum(np.abs(ud), np.abs(vd))),
                          ("rot", np.maximum(np.abs(au), np.abs(av)))):
            acc[name] = max(acc.get(name, 0), int(np.abs(val).max()))
        acc["s_min"], acc["s_max"] = min(acc.get("s_min", 0), int(s.min())), max(acc.get("s_max", 0), int(s.max()))
    return ydm, au >> 12, av >> 12


def cascade(c, signal="composite", chroma="sharp", crawl=True, index=0, decoder="delay", phase=0, acc=None, uv=None):
    """The codes [n, h, w, 3] -> the unclamped R, G, B (the caller clamps them to 0..M, M = `top`).  `uv`, a list, receives (U, V) of step 8."""
    assert decoder in DECODERS
    yd, ur, vr = rows(c, signal, chroma, crawl, index, phase, acc)
    if decoder == "delay":
        yp = partner_rows(c.shape[1])
        u, v = (ur + ur[:, yp] + 1) >> 1, (vr + vr[:, yp] + 1) >> 1
    else:
        u, v = ur, vr
    if uv is not None:
        uv.append((u, v))
    rgb = np.stack([m[0] * yd + m[1] * u + m[2] * v + 32768 for m in TO_RGB], axis=-1)
    if acc is not None and rgb.size:
        acc["last"] = max(acc.get("last", 0), int(np.abs(rgb).max()))
        acc["uv"] = max(acc.get("uv", 0), int(np.abs(u).max()), int(np.abs(v).max()))
    assert rgb.size == 0 or np.abs(rgb).max() <= ACC_MAX
    return rgb >> 16


def pal(frames, signal="composite", chroma="sharp", crawl=True, index=0, decoder="delay", phase=0):
    """frames [n, h, w, 3] uint8 or float16 -> the same shape and dtype: frame i is frame index + i of the stream."""
    frames = np.asarray(frames)
    assert frames.ndim == 4 and index >= 0
    out = np.zeros(frames.shape, frames.dtype)
    n = frames.shape[0]
    step = max(1, (1 << 19) // max(1, int(np.prod(frames.shape[1:]))))           # frames per pass: the int64 temporaries stay small
    for j in range(0, n, step):
        v = cascade(codes(frames[j:j + step]), signal, chroma, crawl, index + j, decoder, phase)
        out[j:j + step] = from_codes(np.clip(v, 0, top(frames.dtype)), frames.dtype.type)
    return out
