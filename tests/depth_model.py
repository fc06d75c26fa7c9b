"""The depth stage in numpy (include/crtfx_depth.h states the arithmetic; this file restates it and nothing else): `widen(u8)` is half(u),
`narrow(f16, dither)` clamps the half to 0..255 (NaN -> 0) and rounds to nearest, ties to even ("none"), or takes floor(v + t[y & 7][x & 7])
with t = (2 * BAYER8 + 1) / 128 ("ordered"), the sum in float32.  Frames are [..., h, w, 3]: (y, x) are the third and second axes from the end."""
import numpy as np


def bayer(n: int) -> np.ndarray:
    """The n x n Bayer index matrix of the recursive 2 x 2 construction: M2 = [0 2; 3 1], M2n = [4M 4M+2; 4M+3 4M+1]."""
    m = np.zeros((1, 1), dtype=np.int64)
    while m.shape[0] < n:
        m = np.block([[4 * m, 4 * m + 2], [4 * m + 3, 4 * m + 1]])
    return m


BAYER8 = bayer(8)
DITHERS = ("none", "ordered")


def thresholds() -> np.ndarray:
    """t[y & 7][x & 7] as float32: odd multiples of 1 / 128 below 1, exact."""
    return ((2 * BAYER8 + 1).astype(np.float32) / np.float32(128.0)).astype(np.float32)


def widen(u8) -> np.ndarray:
    u8 = np.asarray(u8)
    assert u8.dtype == np.uint8
    return u8.astype(np.float16)


def clamp(f16) -> np.ndarray:
    """v = min(max(f, 0), 255) in float32, NaN -> 0."""
    f = np.asarray(f16)
    assert f.dtype == np.float16
    f = f.astype(np.float32)
    with np.errstate(invalid="ignore"):
        v = np.where(f > 0, f, np.float32(0.0))         # NaN, -0, negatives, -inf
        return np.where(v < 255, v, np.float32(255.0)).astype(np.float32)


def narrow(f16, dither: str = "none") -> np.ndarray:
    """[..., h, w, 3] half frames -> uint8 frames."""
    assert dither in DITHERS
    v = clamp(f16)
    if dither == "none":
        return np.rint(v).astype(np.uint8)
    h, w = v.shape[-3], v.shape[-2]
    t = thresholds()[np.arange(h)[:, None] & 7, np.arange(w)[None, :] & 7]          # [h, w]
    s = v + t[:, :, None]                                                           # float32 + float32 -> float32
    assert s.dtype == np.float32
    return np.floor(s).astype(np.uint8)
