"""Host model of the sited source stage (include/crtfx_sited.h): the seven sub-sampled layouts -> RGB with chroma interpolated at siting
"left" or "center", in numpy int64 with the arithmetic written out: the tap tables, D(C), one accumulator, one shift, one clamp.  The
matrices are literals: those of tests/unpack_model.py (8-bit) and the 10-bit source literals of tests/deep_model.py.  Plus a float64
restatement — interpolate in float, then the float matrix, rounded half up — that the integer model is compared with."""
import numpy as np

from tests import deep_model, unpack_model, yuv422_model

SH = 20                                 # 16 fractional bits of the matrix + 4 of the weights (they sum to 16)
LAYOUTS = ("yuv420p", "nv12", "yuv422p", "yuyv422", "uyvy422", "yuv420p10le", "p010le")          # in the order of crtfx_sited_layout
SITINGS = ("left", "center")
DEEP = ("yuv420p10le", "p010le")
V420 = ("yuv420p", "nv12") + DEEP
MATRICES8, OFFSETS8 = unpack_model.MATRICES, unpack_model.OFFSETS
MATRICES10, OFFSETS10 = deep_model.RGB_MATRICES, deep_model.OFFSETS
CASES = sorted(MATRICES8)


def family(layout):
    """The existing model of the layout's replicating stage."""
    return deep_model if layout in DEEP else unpack_model if layout in V420 else yuv422_model


def tables(layout, matrix="bt601", rng="tv"):
    """(m int64 [3, 3], off, the largest output code)"""
    if layout in DEEP:
        return np.array(MATRICES10[(matrix, rng)], dtype=np.int64), OFFSETS10[rng], 1020
    return np.array(MATRICES8[(matrix, rng)], dtype=np.int64), OFFSETS8[rng], 255


def frame_bytes(h, w, layout):
    return family(layout).sizes(h, w, layout)[-1] if layout in yuv422_model.LAYOUTS else family(layout).sizes(h, w)[-1]


def planes(packed, h, w, layout):
    """The samples (Y [h, w], U [rows, cw], V [rows, cw]) int64 of one packed frame, through the existing models' readers."""
    return tuple(np.asarray(p).astype(np.int64) for p in family(layout).planes(packed, h, w, layout))


def h_taps(w, siting):
    """(cx, cxf, hn, hf) per luma column x, written out as the header does."""
    cw = (w + 1) // 2
    cx, cxf, hn, hf = [], [], [], []
    for x in range(w):
        c = x >> 1
        cx.append(c)
        if siting == "left":
            if x % 2 == 0:
                cxf.append(c); hn.append(4); hf.append(0)
            else:
                cxf.append(min(c + 1, cw - 1)); hn.append(2); hf.append(2)
        else:
            assert siting == "center"
            cxf.append(max(c - 1, 0) if x % 2 == 0 else min(c + 1, cw - 1)); hn.append(3); hf.append(1)
    return tuple(np.array(t, dtype=np.int64) for t in (cx, cxf, hn, hf))


def v_taps(h, v420):
    """(cy, cyf, vn, vf) per luma row y."""
    if not v420:
        y = np.arange(h, dtype=np.int64)
        return y, y, np.full(h, 4, dtype=np.int64), np.zeros(h, dtype=np.int64)
    rows = (h + 1) // 2
    cy = [y >> 1 for y in range(h)]
    cyf = [max((y >> 1) - 1, 0) if y % 2 == 0 else min((y >> 1) + 1, rows - 1) for y in range(h)]
    return np.array(cy, dtype=np.int64), np.array(cyf, dtype=np.int64), np.full(h, 3, dtype=np.int64), np.ones(h, dtype=np.int64)


def interpolate(c, h, w, siting, v420):
    """D(C) int64 [h, w] of a chroma plane int64 [rows, cw]: 16 x the interpolated sample."""
    cx, cxf, hn, hf = h_taps(w, siting)
    cy, cyf, vn, vf = v_taps(h, v420)
    c = np.asarray(c, dtype=np.int64)
    near = hn[None, :] * c[cy][:, cx] + hf[None, :] * c[cy][:, cxf]
    far = hn[None, :] * c[cyf][:, cx] + hf[None, :] * c[cyf][:, cxf]
    return vn[:, None] * near + vf[:, None] * far


def live(h, w, layout, siting):
    """bool [h, w]: the pixels with a tap of non-zero weight on another sample than their own.  The others ("left": even columns of a
    4:2:2 frame, and of the first and last row pair's outer rows of a 4:2:0 one; the clamped corners) have equal taps by construction and
    give the replicating stage's bytes."""
    cx, cxf, _, hf = h_taps(w, siting)
    cy, cyf, _, vf = v_taps(h, layout in V420)
    return ((hf > 0) & (cxf != cx))[None, :] | ((vf > 0) & (cyf != cy))[:, None]


def codes_from_planes(y, u, v, layout, siting, m, off, top):
    """The arithmetic on planes of samples: output codes int64 [h, w, 3]."""
    h, w = y.shape
    m = np.asarray(m, dtype=np.int64)
    du, dv = interpolate(u, h, w, siting, layout in V420), interpolate(v, h, w, siting, layout in V420)
    acc = np.stack([16 * m[k, 0] * (y - off[0]) + m[k, 1] * (du - 16 * off[1]) + m[k, 2] * (dv - 16 * off[2]) + (1 << (SH - 1)) for k in range(3)], axis=-1)
    return np.clip(acc >> SH, 0, top)


def codes(packed, h, w, layout, siting="left", matrix="bt601", rng="tv", m=None, off=None):
    """Output codes int64 [h, w, 3] of one packed frame: bytes for the 8-bit layouts, quarter codes for the 10-bit ones.  `m` / `off`
    override the named matrix (the accumulator tests)."""
    tm, toff, top = tables(layout, matrix, rng)
    y, u, v = planes(packed, h, w, layout)
    return codes_from_planes(y, u, v, layout, siting, tm if m is None else m, toff if off is None else off, top)


def unpack(packed, h, w, layout, siting="left", matrix="bt601", rng="tv", m=None, off=None):
    """The RGB frame of one packed frame: uint8 [h, w, 3], or float16 [h, w, 3] on the 0..255 scale (half(q / 4), exact) for a 10-bit layout."""
    q = codes(packed, h, w, layout, siting, matrix, rng, m, off)
    return deep_model.to_half(q) if layout in DEEP else q.astype(np.uint8)


def replicate(packed, h, w, layout, matrix="bt601", rng="tv"):
    """What the replicating stage of the layout gives for the same frame (the existing models)."""
    return family(layout).unpack(packed, h, w, layout, matrix, rng)


def unpack_float(packed, h, w, layout, siting="left", matrix="bt601", rng="tv"):
    """The float restatement: (codes int64 [h, w, 3], the float64 values before rounding): chroma interpolated in float64 (D / 16), the
    float matrix of the layout's family, rounded half up, clamped."""
    _, off, top = tables(layout, matrix, rng)
    f = deep_model.rgb_float_matrix(matrix, rng) if layout in DEEP else unpack_model.float_matrix(matrix, rng)
    y, u, v = planes(packed, h, w, layout)
    d = interpolate(u, h, w, siting, layout in V420).astype(np.float64) / 16.0 - off[1]
    e = interpolate(v, h, w, siting, layout in V420).astype(np.float64) / 16.0 - off[2]
    c = y.astype(np.float64) - off[0]
    raw = np.stack([f[k, 0] * c + f[k, 1] * d + f[k, 2] * e for k in range(3)], axis=-1)
    return np.clip(np.floor(raw + 0.5), 0, top).astype(np.int64), raw


# ---- test frames ----------------------------------------------------------------------------------------------------------------------------

def pack_planes(y, u, v, layout):
    return family(layout).pack_planes(y, u, v, layout)


def images(h, w, layout, seed=0):
    """The three packed test frames of a size in `layout`, uint8 [3, frame_bytes]: random, binary 0 / max, clamp colours plus greys — the
    existing models' `images` (the 4:2:2 ones take the 4:2:0 frames' planes with every chroma row doubled, cut to h rows)."""
    if layout in DEEP:
        return np.stack([deep_model.relayout(p, h, w, layout) for p in deep_model.images(h, w, seed)])
    base = unpack_model.images(h, w, seed)
    if layout in V420:
        return np.stack([unpack_model.relayout(p, h, w, layout) for p in base])
    out = []
    rows = np.arange(h) >> 1
    rng = np.random.default_rng(77 * h + w + seed)
    for i, p in enumerate(base):
        y, u, v = unpack_model.planes(p, h, w, "yuv420p")
        u, v = u[rows].copy(), v[rows].copy()
        if i < 2:                                                               # random / binary: the doubled rows differ again
            pick = rng.integers(0, 2, u.shape).astype(bool)
            u, v = np.where(pick, u, u[::-1]), np.where(pick, v, v[::-1])
        out.append(yuv422_model.pack_planes(y, u, v, layout))
    return np.stack(out)
