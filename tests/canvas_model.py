"""The geometry stage in numpy (include/crtfx_canvas.h): a window of a frame placed on a canvas of a fill colour, and the two integer fit
rules restated.  Frames are [..., h, w, 3] arrays of any dtype; samples move as they are."""
import numpy as np


def canvas(src, dst_size, window=None, at=(0, 0), fill=(0, 0, 0)):
    """dst[..., y, x, c] = src[..., win_y + y - dst_y, win_x + x - dst_x, c] inside the placed window, fill[c] elsewhere.  `fill` holds
    values of src's dtype (for float16 frames: halves)."""
    src = np.asarray(src)
    wy, wx, wh, ww = (0, 0) + src.shape[-3:-1] if window is None else window
    assert 0 <= wy and 0 <= wx and wh >= 1 and ww >= 1 and wy + wh <= src.shape[-3] and wx + ww <= src.shape[-2]
    assert 0 <= at[0] and 0 <= at[1] and at[0] + wh <= dst_size[0] and at[1] + ww <= dst_size[1]
    out = np.empty(src.shape[:-3] + tuple(dst_size) + (3,), dtype=src.dtype)
    out[...] = np.asarray(fill, dtype=src.dtype)
    out[..., at[0]:at[0] + wh, at[1]:at[1] + ww, :] = src[..., wy:wy + wh, wx:wx + ww, :]
    return out


def crop(src, window):
    return canvas(src, window[2:], window=window)


def rdiv(a, b):
    return (2 * a + b) // (2 * b)


def fit_pad(size, deliver):
    (h, w), (dh, dw) = size, deliver
    if w * dh <= h * dw:
        ih, iw = dh, min(max(rdiv(w * dh, h), 1), dw)
    else:
        iw, ih = dw, min(max(rdiv(h * dw, w), 1), dh)
    return (ih, iw), ((dh - ih) // 2, (dw - iw) // 2)


def fit_crop(size, deliver):
    (h, w), (dh, dw) = size, deliver
    if w * dh >= h * dw:
        ch, cw = h, min(max(rdiv(h * dw, dh), 1), w)
    else:
        cw, ch = w, min(max(rdiv(w * dh, dw), 1), h)
    return (h - ch) // 2, (w - cw) // 2, ch, cw
