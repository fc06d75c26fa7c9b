"""Host model of the field-paired 4:2:0 source stage (include/crtfx_field420.h): yuv420p / nv12 / yuv420p10le / p010le -> RGB with every
luma row taking chroma from rows of its own field, in numpy int64 with the arithmetic written out: the vertical taps row by row, the
horizontal ones of tests/sited_model.py, D(C), one accumulator, one shift, one clamp.  The planes are read through the existing models'
readers and the matrices are their literals (tests/unpack_model.py, tests/deep_model.py).  Plus a float64 restatement — interpolate in
float, then the float matrix, rounded half up — that the integer model is compared with."""
import numpy as np

from tests import deep_model, sited_model, unpack_model

SH = 21                                 # 16 fractional bits of the matrix + 5 of the weights (they sum to 32)
LAYOUTS = ("yuv420p", "nv12", "yuv420p10le", "p010le")           # in the order of crtfx_field420_layout
CHROMAS = ("replicate", "left", "center")                        # in the order of crtfx_field420_chroma
DEEP = ("yuv420p10le", "p010le")
MATRICES8, OFFSETS8 = unpack_model.MATRICES, unpack_model.OFFSETS
MATRICES10, OFFSETS10 = deep_model.RGB_MATRICES, deep_model.OFFSETS
CASES = sorted(MATRICES8)


def family(layout):
    """The existing model of the layout's replicating stage."""
    return deep_model if layout in DEEP else unpack_model


def tables(layout, matrix="bt601", rng="tv"):
    """(m int64 [3, 3], off, the largest output code)"""
    if layout in DEEP:
        return np.array(MATRICES10[(matrix, rng)], dtype=np.int64), OFFSETS10[rng], 1020
    return np.array(MATRICES8[(matrix, rng)], dtype=np.int64), OFFSETS8[rng], 255


def frame_bytes(h, w, layout):
    return family(layout).sizes(h, w)[-1]


def planes(packed, h, w, layout):
    """The samples (Y [h, w], U [ch, cw], V [ch, cw]) int64 of one packed frame, through the existing models' readers."""
    return tuple(np.asarray(p).astype(np.int64) for p in family(layout).planes(packed, h, w, layout))


def pack_planes(y, u, v, layout):
    return family(layout).pack_planes(np.asarray(y), np.asarray(u), np.asarray(v), layout)


def v_taps(h, chroma):
    """(cy, cyf, vn, vf) per luma row y, FRAME chroma rows, written out row by row as the header does."""
    assert h % 2 == 0 and h >= 4
    ch = h // 2
    cy, cyf, vn, vf = [], [], [], []
    for y in range(h):
        f = y & 1                       # the field of the row
        k = y >> 1                      # its row inside the field
        j = k >> 1                      # the field's chroma row above or at it
        n_f = (ch + 1 - f) // 2         # the chroma rows the field owns
        far = j - 1 if k % 2 == 0 else j + 1
        near_row = min(max(j, 0), n_f - 1)
        far_row = min(max(far, 0), n_f - 1)
        if chroma == "replicate":
            wn, wf = 8, 0
        elif f == 0:                    # top field: the chroma row sits a quarter field row below its first luma row
            wn, wf = (7, 1) if k % 2 == 0 else (5, 3)
        else:                           # bottom field: three quarters below
            wn, wf = (5, 3) if k % 2 == 0 else (7, 1)
        cy.append(2 * near_row + f)
        cyf.append(2 * far_row + f)
        vn.append(wn)
        vf.append(wf)
    return tuple(np.array(t, dtype=np.int64) for t in (cy, cyf, vn, vf))


def h_taps(w, chroma):
    """(cx, cxf, hn, hf) per luma column x: those of the sited stage for "left" and "center", the pixel's own sample for "replicate"."""
    if chroma == "replicate":
        cx = np.arange(w, dtype=np.int64) >> 1
        return cx, cx, np.full(w, 4, dtype=np.int64), np.zeros(w, dtype=np.int64)
    return sited_model.h_taps(w, chroma)


def interpolate(c, h, w, chroma):
    """D(C) int64 [h, w] of a chroma plane int64 [h / 2, cw]: 32 x the interpolated sample."""
    cx, cxf, hn, hf = h_taps(w, chroma)
    cy, cyf, vn, vf = v_taps(h, chroma)
    c = np.asarray(c, dtype=np.int64)
    near = hn[None, :] * c[cy][:, cx] + hf[None, :] * c[cy][:, cxf]
    far = hn[None, :] * c[cyf][:, cx] + hf[None, :] * c[cyf][:, cxf]
    return vn[:, None] * near + vf[:, None] * far


def codes_from_planes(y, u, v, layout, chroma, m, off, top):
    """The arithmetic on planes of samples: output codes int64 [h, w, 3]."""
    h, w = y.shape
    m = np.asarray(m, dtype=np.int64)
    du, dv = interpolate(u, h, w, chroma), interpolate(v, h, w, chroma)
    acc = np.stack([32 * m[k, 0] * (y - off[0]) + m[k, 1] * (du - 32 * off[1]) + m[k, 2] * (dv - 32 * off[2]) + (1 << (SH - 1)) for k in range(3)], axis=-1)
    return np.clip(acc >> SH, 0, top)


def codes(packed, h, w, layout, chroma="replicate", matrix="bt601", rng="tv", m=None, off=None):
    """Output codes int64 [h, w, 3] of one packed frame: bytes for the 8-bit layouts, quarter codes for the 10-bit ones.  `m` / `off`
    override the named matrix."""
    tm, toff, top = tables(layout, matrix, rng)
    y, u, v = planes(packed, h, w, layout)
    return codes_from_planes(y, u, v, layout, chroma, tm if m is None else m, toff if off is None else off, top)


def unpack(packed, h, w, layout, chroma="replicate", matrix="bt601", rng="tv", m=None, off=None):
    """The RGB frame of one packed frame: uint8 [h, w, 3], or float16 [h, w, 3] on the 0..255 scale (half(q / 4), exact) for a 10-bit layout."""
    q = codes(packed, h, w, layout, chroma, matrix, rng, m, off)
    return deep_model.to_half(q) if layout in DEEP else q.astype(np.uint8)


def unpack_batch(packed, h, w, layout, chroma="replicate", matrix="bt601", rng="tv"):
    return np.stack([unpack(p, h, w, layout, chroma, matrix, rng) for p in packed])


def progressive(packed, h, w, layout, chroma="replicate", matrix="bt601", rng="tv"):
    """What the progressive source stage of the layout gives for the same frame: the replicating one, or the sited one under "left" / "center"."""
    if chroma == "replicate":
        return family(layout).unpack(packed, h, w, layout, matrix, rng)
    return sited_model.unpack(packed, h, w, layout, chroma, matrix, rng)


def field_frame(packed, h, w, layout, f):
    """Field f of a packed frame as an h/2 x w packed frame of its own: luma rows f, f + 2, ..., chroma rows f, f + 2, ...; h % 4 == 0."""
    assert h % 4 == 0
    y, u, v = planes(packed, h, w, layout)
    return pack_planes(y[f::2], u[f::2], v[f::2], layout)


def weave_of_fields(packed, h, w, layout, matrix="bt601", rng="tv"):
    """The existing replicating model run on each field as a frame of its own, the two results woven."""
    top = family(layout).unpack(field_frame(packed, h, w, layout, 0), h // 2, w, layout, matrix, rng)
    out = np.empty((h, w, 3), dtype=top.dtype)
    out[0::2] = top
    out[1::2] = family(layout).unpack(field_frame(packed, h, w, layout, 1), h // 2, w, layout, matrix, rng)
    return out


def unpack_float(packed, h, w, layout, chroma="replicate", matrix="bt601", rng="tv"):
    """The float restatement: (codes int64 [h, w, 3], the float64 values before rounding): chroma interpolated in float64 (D / 32), the
    float matrix of the layout's family, rounded half up, clamped."""
    _, off, top = tables(layout, matrix, rng)
    f = deep_model.rgb_float_matrix(matrix, rng) if layout in DEEP else unpack_model.float_matrix(matrix, rng)
    y, u, v = planes(packed, h, w, layout)
    d = interpolate(u, h, w, chroma).astype(np.float64) / 32.0 - off[1]
    e = interpolate(v, h, w, chroma).astype(np.float64) / 32.0 - off[2]
    c = y.astype(np.float64) - off[0]
    raw = np.stack([f[k, 0] * c + f[k, 1] * d + f[k, 2] * e for k in range(3)], axis=-1)
    return np.clip(np.floor(raw + 0.5), 0, top).astype(np.int64), raw


# ---- test frames ----------------------------------------------------------------------------------------------------------------------------

def images(h, w, layout, seed=0):
    """The three packed test frames of a size in `layout`, uint8 [3, frame_bytes]: random, binary 0 / max, clamp colours plus greys — the
    existing models' `images`."""
    return sited_model.images(h, w, layout, seed)


def two_colour_frame(h, w, layout, top_yuv, bottom_yuv):
    """A packed frame whose top field is one flat colour and whose bottom field another, as an interlaced encoder sub-samples it: luma
    rows and chroma rows alternate between the two colours."""
    y = np.empty((h, w), dtype=np.int64)
    u = np.empty((h // 2, (w + 1) // 2), dtype=np.int64)
    v = np.empty_like(u)
    for f, (yy, uu, vv) in enumerate((top_yuv, bottom_yuv)):
        y[f::2], u[f::2], v[f::2] = yy, uu, vv
    return pack_planes(y, u, v, layout)
