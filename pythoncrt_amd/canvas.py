"""`Canvas` — `crop` and `pad` on the device: one window of RGB frames (uint8 or float16) of one size in HBM is placed into frames of
another, the rest filled with a colour (include/crtfx_canvas.h), several frames per launch.  Nothing is computed: samples move as bits.
`fit_pad` / `fit_crop` are the integer rules of `scale=...:force_original_aspect_ratio=decrease` + `pad` and `...=increase` + `crop`: the
size a frame takes inside a delivery of another aspect, and the window of a frame that has the delivery's aspect."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

from . import _lib
from ._stage import FramePlan, pix_format


def _rdiv(a: int, b: int) -> int:
    """a / b rounded to nearest, halves up, in integers."""
    return (2 * a + b) // (2 * b)


def fit_pad(size: Tuple[int, int], deliver: Tuple[int, int]):
    """((ih, iw), (dy, dx)): the largest size of the (h, w) frame's aspect inside the (dh, dw) delivery, and where it sits centred."""
    (h, w), (dh, dw) = (int(size[0]), int(size[1])), (int(deliver[0]), int(deliver[1]))
    if w * dh <= h * dw:
        ih, iw = dh, max(1, min(dw, _rdiv(w * dh, h)))
    else:
        ih, iw = max(1, min(dh, _rdiv(h * dw, w))), dw
    return (ih, iw), ((dh - ih) // 2, (dw - iw) // 2)


def fit_crop(size: Tuple[int, int], deliver: Tuple[int, int]):
    """(y, x, ch, cw): the largest centred window of the (h, w) frame that has the (dh, dw) delivery's aspect."""
    (h, w), (dh, dw) = (int(size[0]), int(size[1])), (int(deliver[0]), int(deliver[1]))
    if w * dh >= h * dw:
        ch, cw = h, max(1, min(w, _rdiv(h * dw, dh)))
    else:
        ch, cw = max(1, min(h, _rdiv(w * dh, dw))), w
    return (h - ch) // 2, (w - cw) // 2, ch, cw


class Canvas(FramePlan):
    """plan = Canvas(device, (src_h, src_w), (dst_h, dst_w), window=(y, x, h, w), at=(dst_y, dst_x), fill=(r, g, b));
    out = plan.run(frames[n, src_h, src_w, 3]) -> [n, dst_h, dst_w, 3] of the same dtype: the window placed at `at`, `fill` elsewhere.
    `window=None` is the whole source; `fill` is 0..255 per channel (for float16 frames the half of that value); `dtype` is torch.uint8
    unless given.  `frames` and `out` are tensors on `device` whose frames are contiguous (the batch stride is free: slices of larger
    tensors are fine).  The work is enqueued on the current stream of `device`; nothing synchronises.  plan.plan() is
    crtfx_canvas_last_plan as a dictionary, e.g. {"canvas": "k_canvas<u8,vec>", "frames": "5"}."""
    _family = "canvas"
    _force_option = _lib.CANVAS_OPT_FORCE_GENERAL

    def __init__(self, device, src_size: Tuple[int, int], dst_size: Tuple[int, int], window: Optional[Tuple[int, int, int, int]] = None,
                 at: Tuple[int, int] = (0, 0), fill: Tuple[int, int, int] = (0, 0, 0), dtype=None, force_general: bool = False):
        import numpy as np
        self._open(device)
        self.dtype, pix_fmt = pix_format(dtype, error=lambda text: _lib.CrtfxError(_lib.E_UNSUPPORTED, text))
        self.src_size = (int(src_size[0]), int(src_size[1]))
        self.dst_size = (int(dst_size[0]), int(dst_size[1]))
        self.window = (0, 0) + self.src_size if window is None else tuple(int(v) for v in window)
        self.at = (int(at[0]), int(at[1]))
        self.fill = tuple(int(v) for v in fill)
        if len(self.window) != 4 or len(self.fill) != 3 or min(self.fill) < 0 or max(self.fill) > 255:
            raise ValueError(f"window is (y, x, h, w) and fill three values 0..255, got {window!r} and {fill!r}")
        codes = np.array(self.fill, dtype=np.float16).view(np.uint16) if pix_fmt == _lib.PIX_F16 else np.array(self.fill, dtype=np.uint16)
        self._create(pix_fmt, *self.src_size, *self.window, *self.dst_size, *self.at, (ctypes.c_uint16 * 3)(*(int(c) for c in codes)))
        self._frames(self.src_size + (self.dtype,), self.dst_size + (self.dtype,))
        if force_general:
            self.force_general = True
