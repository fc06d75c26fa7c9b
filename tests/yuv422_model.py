"""Host model of the 8-bit 4:2:2 pair (include/crtfx_422.h): yuv422p / yuyv422 / uyvy422 -> RGB and RGB -> the same three layouts in numpy
int64, the arithmetic written out.  The matrices are the literals of tests/unpack_model.py (source) and tests/yuv_model.py (egress), which
tests/test_unpack_tables.py / tests/test_egress_tables.py hold pythoncrt_amd.tables to; plus a float64 restatement of each direction that
the integer models are compared with."""
import numpy as np

from tests import unpack_model, yuv_model

SH = 16
RGB_MATRICES, YUV_MATRICES = unpack_model.MATRICES, yuv_model.MATRICES
OFFSETS = unpack_model.OFFSETS
assert OFFSETS == yuv_model.OFFSETS
CASES = sorted(RGB_MATRICES)
LAYOUTS = ("yuv422p", "yuyv422", "uyvy422")
MACROPIXEL = {"yuyv422": (0, 2, 1, 3), "uyvy422": (1, 3, 0, 2)}          # byte positions of Y0, Y1, U, V


def sizes(h, w, layout):
    """(cw, frame_bytes)"""
    cw = (w + 1) // 2
    assert layout in LAYOUTS
    return cw, (h * w + 2 * h * cw if layout == "yuv422p" else 4 * h * cw)


def planes(packed, h, w, layout):
    """(Y [h, w], U [h, cw], V [h, cw]) uint8 copies of one packed frame; the pad byte of an odd-width packed row is not among them."""
    cw, fb = sizes(h, w, layout)
    p = np.asarray(packed).reshape(-1)
    assert p.shape == (fb,) and p.dtype == np.uint8
    if layout == "yuv422p":
        return p[:h * w].reshape(h, w).copy(), p[h * w:h * w + h * cw].reshape(h, cw).copy(), p[h * w + h * cw:].reshape(h, cw).copy()
    y0, y1, u, v = MACROPIXEL[layout]
    mp = p.reshape(h, cw, 4)
    y = np.stack([mp[..., y0], mp[..., y1]], axis=2).reshape(h, 2 * cw)[:, :w]
    return y.copy(), mp[..., u].copy(), mp[..., v].copy()


def pack_planes(y, u, v, layout):
    """The inverse of `planes`: uint8 [frame_bytes]; the pad byte of an odd-width packed row is a copy of the row's last Y."""
    h, w = y.shape
    cw, fb = sizes(h, w, layout)
    assert u.shape == v.shape == (h, cw)
    if layout == "yuv422p":
        out = np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]).astype(np.uint8)
    else:
        y0, y1, pu, pv = MACROPIXEL[layout]
        ypad = np.concatenate([y, y[:, -1:]], axis=1)[:, :2 * cw]
        mp = np.zeros((h, cw, 4), dtype=np.uint8)
        mp[..., y0], mp[..., y1], mp[..., pu], mp[..., pv] = ypad[:, 0::2], ypad[:, 1::2], u, v
        out = mp.reshape(-1)
    assert out.shape == (fb,)
    return out


def relayout(packed, h, w, src_layout, layout):
    """A frame given in `src_layout`, in `layout` (the same samples)."""
    return pack_planes(*planes(packed, h, w, src_layout), layout)


# ---- source ---------------------------------------------------------------------------------------------------------------------------------

def terms(packed, h, w, layout, rng):
    """(c, d, e) int64 [h, w] each: the samples less their offsets, chroma replicated over its horizontal pair (an odd edge reads the last sample)."""
    y, u, v = planes(packed, h, w, layout)
    off = OFFSETS[rng]
    xx = np.arange(w) >> 1
    return y.astype(np.int64) - off[0], u.astype(np.int64)[:, xx] - off[1], v.astype(np.int64)[:, xx] - off[2]


def convert_yuv(c, d, e, matrix="bt601", rng="tv"):
    """The source arithmetic on arrays of (c, d, e): uint8 [..., 3]."""
    m = np.array(RGB_MATRICES[(matrix, rng)], dtype=np.int64)
    acc = np.stack([m[k, 0] * c + m[k, 1] * d + m[k, 2] * e + (1 << (SH - 1)) for k in range(3)], axis=-1)
    assert acc.min() >= -2 ** 31 and acc.max() < 2 ** 31
    return np.clip(acc >> SH, 0, 255).astype(np.uint8)


def unpack(packed, h, w, layout, matrix="bt601", rng="tv"):
    """uint8 [h, w, 3] RGB of one packed uint8 frame."""
    return convert_yuv(*terms(packed, h, w, layout, rng), matrix, rng)


def unpack_float(packed, h, w, layout, matrix="bt601", rng="tv"):
    """The float restatement of the source: (uint8 [h, w, 3], the float64 values before rounding): round-half-up(F . (c, d, e)), clamped."""
    f = unpack_model.float_matrix(matrix, rng)
    c, d, e = (x.astype(np.float64) for x in terms(packed, h, w, layout, rng))
    raw = np.stack([f[k, 0] * c + f[k, 1] * d + f[k, 2] * e for k in range(3)], axis=-1)
    return np.clip(np.floor(raw + 0.5), 0, 255).astype(np.uint8), raw


# ---- egress ---------------------------------------------------------------------------------------------------------------------------------

def pair_sum(rgb):
    """S[y][cx]: the two samples under a chroma sample, the last column replicated at an odd edge.  int64 [h, cw, 3]."""
    w = rgb.shape[1]
    x0 = np.arange(0, w, 2)
    x1 = np.minimum(x0 + 1, w - 1)
    a = rgb.astype(np.int64)
    return a[:, x0] + a[:, x1]


def convert(rgb, matrix="bt601", rng="tv"):
    """(Y [h, w], U [h, cw], V [h, cw]) uint8 of one uint8 h x w x 3 frame."""
    m, off = np.array(YUV_MATRICES[(matrix, rng)], dtype=np.int64), OFFSETS[rng]
    acc_y = rgb.astype(np.int64) @ m[0] + (off[0] << SH) + (1 << (SH - 1))
    s = pair_sum(rgb)
    acc_u = s @ m[1] + (off[1] << (SH + 1)) + (1 << SH)
    acc_v = s @ m[2] + (off[2] << (SH + 1)) + (1 << SH)
    for acc in (acc_y, acc_u, acc_v):
        assert acc.min() >= 0 and acc.max() < 2 ** 31
    return (np.clip(acc_y >> SH, 0, 255).astype(np.uint8), np.clip(acc_u >> (SH + 1), 0, 255).astype(np.uint8),
            np.clip(acc_v >> (SH + 1), 0, 255).astype(np.uint8))


def pack(rgb, layout, matrix="bt601", rng="tv"):
    """The bytes of one uint8 h x w x 3 frame in `layout`: uint8 [frame_bytes]."""
    return pack_planes(*convert(rgb, matrix, rng), layout)


def convert_float(rgb, matrix="bt601", rng="tv"):
    """The float restatement of the egress: ((Y, U, V) uint8, (y, u, v) the float64 values before rounding); chroma from the float mean S / 2."""
    f, off = yuv_model.float_matrix(matrix, rng), OFFSETS[rng]
    mean = pair_sum(rgb).astype(np.float64) / 2.0
    raw = (rgb.astype(np.float64) @ f[0] + off[0], mean @ f[1] + off[1], mean @ f[2] + off[2])
    return tuple(np.clip(np.floor(r + 0.5), 0, 255).astype(np.uint8) for r in raw), raw


# ---- test frames ----------------------------------------------------------------------------------------------------------------------------

def sources(h, w, layout, n=3, seed=0):
    """n packed source frames of random bytes over all of 0..255 (both clamps live), uint8 [n, frame_bytes]."""
    _, fb = sizes(h, w, layout)
    return np.random.default_rng(7000 * h + 7 * w + seed).integers(0, 256, (n, fb), dtype=np.uint8)


def frames(h, w, n=3, seed=0):
    """n random RGB frames, uint8 [n, h, w, 3]."""
    return np.random.default_rng(9000 * h + 9 * w + seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
