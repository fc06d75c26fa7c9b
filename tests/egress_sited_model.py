"""Host model of the sited egress stage (include/crtfx_egress_sited.h): RGB -> the seven sub-sampled layouts with chroma filtered onto siting
"left" or "center", in numpy int64 with the arithmetic written out: the x / y index tables, H, S, one accumulator, one shift, one clamp.
The matrices are literals: those of tests/yuv_model.py (8-bit; tests/yuv422_model.py uses the same) and the 10-bit egress literals of
tests/deep_model.py; the quantiser is deep_model.quantise; the layout writers are those models'.  Plus a float64 restatement — filter in
float, then the float matrix, rounded half up — that the integer model is compared with."""
import numpy as np

from tests import deep_model, yuv422_model, yuv_model

SH = 16
LAYOUTS = ("yuv420p", "nv12", "yuv422p", "yuyv422", "uyvy422", "yuv420p10le", "p010le")          # in the order of crtfx_sited_layout
SITINGS = ("left", "center")
WEIGHTS = {"left": (1, 2, 1), "center": (0, 2, 2)}                                                # (wl, w0, wr) in quarters
DEEP = ("yuv420p10le", "p010le")
V420 = ("yuv420p", "nv12") + DEEP
MATRICES8, OFFSETS8 = yuv_model.MATRICES, yuv_model.OFFSETS
MATRICES10, OFFSETS10 = deep_model.YUV_MATRICES, deep_model.OFFSETS
assert yuv422_model.YUV_MATRICES is MATRICES8
CASES = sorted(MATRICES8)


def tables(layout, matrix="bt601", rng="tv"):
    """(m int64 [3, 3], off, T the largest sample)"""
    if layout in DEEP:
        return np.array(MATRICES10[(matrix, rng)], dtype=np.int64), OFFSETS10[rng], 1023
    return np.array(MATRICES8[(matrix, rng)], dtype=np.int64), OFFSETS8[rng], 255


def frame_bytes(h, w, layout):
    if layout in yuv422_model.LAYOUTS:
        return yuv422_model.sizes(h, w, layout)[-1]
    return (deep_model if layout in DEEP else yuv_model).sizes(h, w)[-1]


def x_taps(w):
    """(xl, x0, xr) per chroma column cx, written out as the header does."""
    xl, x0, xr = [], [], []
    for cx in range((w + 1) // 2):
        x0.append(2 * cx)
        xl.append(max(2 * cx - 1, 0))
        xr.append(min(2 * cx + 1, w - 1))
    return tuple(np.array(t, dtype=np.int64) for t in (xl, x0, xr))


def y_taps(h, v420):
    """(y0, y1) per chroma row: the two rows of a 4:2:0 sample (the last one twice at an odd edge); 4:2:2 has the one row (y1 = y0, unused)."""
    if not v420:
        y = np.arange(h, dtype=np.int64)
        return y, y
    y0 = [2 * cy for cy in range((h + 1) // 2)]
    y1 = [min(2 * cy + 1, h - 1) for cy in range((h + 1) // 2)]
    return np.array(y0, dtype=np.int64), np.array(y1, dtype=np.int64)


def pixel_codes(rgb, layout):
    """p int64 [h, w, 3]: the uint8 channel values, or the quarter codes of a float16 frame (deep_model.quantise)."""
    if layout in DEEP:
        return deep_model.quantise(np.asarray(rgb))
    assert np.asarray(rgb).dtype == np.uint8
    return np.asarray(rgb).astype(np.int64)


def filter_sum(p, layout, siting):
    """S int64 [rows, cw, 3] of per-pixel codes p [h, w, 3]: H over the three columns, summed over the two rows of a 4:2:0 sample."""
    h, w = p.shape[:2]
    wl, w0, wr = WEIGHTS[siting]
    xl, x0, xr = x_taps(w)
    hsum = wl * p[:, xl] + w0 * p[:, x0] + wr * p[:, xr]                          # H[y][cx]
    if layout not in V420:
        return hsum
    y0, y1 = y_taps(h, True)
    return hsum[y0] + hsum[y1]


def convert_codes(p, layout, siting="left", matrix="bt601", rng="tv", m=None, off=None):
    """(Y [h, w], U [rows, cw], V [rows, cw]) int64 samples of per-pixel codes p.  `m` / `off` override the named matrix."""
    tm, toff, top = tables(layout, matrix, rng)
    m = tm if m is None else np.asarray(m, dtype=np.int64).reshape(3, 3)
    off = toff if off is None else off
    csh = SH + (3 if layout in V420 else 2)
    acc_y = p @ m[0] + (off[0] << SH) + (1 << (SH - 1))
    s = filter_sum(p, layout, siting)
    acc_u = s @ m[1] + (off[1] << csh) + (1 << (csh - 1))
    acc_v = s @ m[2] + (off[2] << csh) + (1 << (csh - 1))
    for acc in (acc_y, acc_u, acc_v):
        assert acc.min() >= 0 and acc.max() < 2 ** 31
    return np.clip(acc_y >> SH, 0, top), np.clip(acc_u >> csh, 0, top), np.clip(acc_v >> csh, 0, top)


def write(y, u, v, layout):
    """The frame's bytes from its samples, through the existing models' writers: uint8 [frame_bytes]."""
    if layout in DEEP:
        return deep_model.pack_planes(y, u, v, layout)
    if layout in yuv422_model.LAYOUTS:
        return yuv422_model.pack_planes(y.astype(np.uint8), u.astype(np.uint8), v.astype(np.uint8), layout)
    y, u, v = (a.astype(np.uint8) for a in (y, u, v))
    if layout == "nv12":                                                           # as yuv_model.pack writes them
        return np.concatenate([y.reshape(-1), np.stack([u, v], axis=2).reshape(-1)])
    assert layout == "yuv420p"
    return np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)])


def pack(rgb, layout, siting="left", matrix="bt601", rng="tv", m=None, off=None):
    """The bytes of one h x w x 3 frame (uint8, or float16 for a 10-bit layout) in `layout`: uint8 [frame_bytes]."""
    return write(*convert_codes(pixel_codes(rgb, layout), layout, siting, matrix, rng, m, off), layout)


def box(rgb, layout, matrix="bt601", rng="tv"):
    """What the box stage of the layout writes for the same frame (the existing models)."""
    if layout in DEEP:
        return deep_model.pack(rgb, layout, matrix, rng)
    if layout in yuv422_model.LAYOUTS:
        return yuv422_model.pack(rgb, layout, matrix, rng)
    return yuv_model.pack(rgb, layout, matrix, rng)


def samples(packed, h, w, layout):
    """(Y, U, V) int64 of a packed frame, through the existing models' readers."""
    if layout in DEEP:
        return deep_model.planes(packed, h, w, layout)
    if layout in yuv422_model.LAYOUTS:
        return tuple(a.astype(np.int64) for a in yuv422_model.planes(packed, h, w, layout))
    from tests import unpack_model
    return tuple(np.asarray(a).astype(np.int64) for a in unpack_model.planes(packed, h, w, layout))


def float_matrix(layout, matrix, rng):
    return deep_model.yuv_float_matrix(matrix, rng) if layout in DEEP else yuv_model.float_matrix(matrix, rng)


def convert_float(p, layout, siting="left", matrix="bt601", rng="tv"):
    """The float restatement behind the per-pixel codes: ((Y, U, V) int64, the float64 values before rounding): the filtered value
    S / 8 (4:2:0) or S / 4 (4:2:2) in float64, the float matrix of the layout's family, rounded half up, clamped."""
    _, off, top = tables(layout, matrix, rng)
    f = float_matrix(layout, matrix, rng)
    mean = filter_sum(p, layout, siting).astype(np.float64) / (8.0 if layout in V420 else 4.0)
    raw = (p.astype(np.float64) @ f[0] + off[0], mean @ f[1] + off[1], mean @ f[2] + off[2])
    return tuple(np.clip(np.floor(r + 0.5), 0, top).astype(np.int64) for r in raw), raw


# ---- test frames ----------------------------------------------------------------------------------------------------------------------------

def images(h, w, layout, seed=0):
    """The three RGB test frames of a size for `layout`, [3, h, w, 3]: the existing family models' — uint8 random / binary / clamp colours
    plus greys (yuv_model.images), or for a 10-bit layout the float16 frames deep_model gives for ITS three packed test frames (random,
    binary, palette: quarter codes over all of 0..1020; the other half patterns are the quantiser tests')."""
    if layout in DEEP:
        return np.stack([deep_model.unpack(p, h, w) for p in deep_model.images(h, w, seed)])
    return yuv_model.images(h, w, seed)
