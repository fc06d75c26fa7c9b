"""Host model of the field-paired 4:2:0 egress stage (include/crtfx_egress_field420.h): RGB -> yuv420p / nv12 / yuv420p10le / p010le with
every chroma sample formed from luma rows of its own field, in numpy int64 with the arithmetic written out: the vertical tap table chroma
row by chroma row, the x taps of tests/egress_sited_model.py, H, S, one accumulator, one shift, one clamp.  The matrices, the per-pixel
codes and the layout writers are that model's (and through it tests/yuv_model.py's and tests/deep_model.py's).  Plus a float64
restatement — filter in float, then the float matrix, rounded half up — that the integer model is compared with."""
import numpy as np

from tests import deep_model, yuv_model
from tests import egress_sited_model as sited

SH = 16
CSH = SH + 6                                                     # the weights of a chroma sum: 4 (horizontal) * 16 (vertical) = 64
LAYOUTS = ("yuv420p", "nv12", "yuv420p10le", "p010le")           # in the order of crtfx_field420_layout
CHROMAS = ("center", "left")                                     # in the order of crtfx_egress_field420_chroma
DEEP = sited.DEEP
H_WEIGHTS = sited.WEIGHTS                                        # (wl, w0, wr) in quarters
V_WEIGHTS = {"center": ((0, 8, 8, 0), (0, 8, 8, 0)),             # [field]: (v_0 .. v_3) in sixteenths over field rows 2i - 1 .. 2i + 2
             "left": ((3, 7, 5, 1), (1, 5, 7, 3))}
SITING = {"center": (0.5, 0.5), "left": (0.25, 0.75)}            # [field]: field rows below field row 2i
MATRICES8, OFFSETS8 = sited.MATRICES8, sited.OFFSETS8
MATRICES10, OFFSETS10 = sited.MATRICES10, sited.OFFSETS10
CASES = sited.CASES
tables, frame_bytes, x_taps, pixel_codes, write, samples, float_matrix, images = (
    sited.tables, sited.frame_bytes, sited.x_taps, sited.pixel_codes, sited.write, sited.samples, sited.float_matrix, sited.images)


def limit(layout):
    """The accumulators of the layout stay in [0, limit): 2^31 for 8 bits (and every Y), 2^32 for the 10-bit chroma rows."""
    return 2 ** 32 if layout in DEEP else 2 ** 31


def v_taps(h):
    """Per chroma row c: (the field f, the four FRAME rows of its taps), written out as the header does."""
    assert h % 4 == 0 and h >= 4
    ch = h // 2                         # chroma rows, and the luma rows of one field
    out = []
    for c in range(ch):
        f = c & 1                       # the field of the chroma row
        i = c >> 1                      # its chroma row inside the field
        rows = []
        for t in range(4):
            k = min(max(2 * i - 1 + t, 0), ch - 1)      # the field row, clamped
            rows.append(2 * k + f)
        out.append((f, tuple(rows)))
    return out


def filter_sum(p, chroma):
    """S int64 [h / 2, cw, 3] of per-pixel codes p [h, w, 3]."""
    h, w = p.shape[:2]
    wl, w0, wr = H_WEIGHTS[chroma]
    xl, x0, xr = x_taps(w)
    hsum = wl * p[:, xl] + w0 * p[:, x0] + wr * p[:, xr]                          # H[y][cx]
    s = np.zeros((h // 2,) + hsum.shape[1:], dtype=np.int64)
    for c, (f, rows) in enumerate(v_taps(h)):
        for t in range(4):
            s[c] += V_WEIGHTS[chroma][f][t] * hsum[rows[t]]
    return s


def accumulators(p, layout, chroma="center", matrix="bt601", rng="tv", m=None, off=None):
    """(acc_y [h, w], acc_u, acc_v [h / 2, cw]) int64, before the shift."""
    tm, toff, _ = tables(layout, matrix, rng)
    m = tm if m is None else np.asarray(m, dtype=np.int64).reshape(3, 3)
    off = toff if off is None else off
    s = filter_sum(p, chroma)
    return (p @ m[0] + (off[0] << SH) + (1 << (SH - 1)), s @ m[1] + (off[1] << CSH) + (1 << (CSH - 1)), s @ m[2] + (off[2] << CSH) + (1 << (CSH - 1)))


def convert_codes(p, layout, chroma="center", matrix="bt601", rng="tv", m=None, off=None):
    """(Y [h, w], U [h / 2, cw], V [h / 2, cw]) int64 samples of per-pixel codes p.  `m` / `off` override the named matrix."""
    top = tables(layout)[2]
    acc_y, acc_u, acc_v = accumulators(p, layout, chroma, matrix, rng, m, off)
    assert acc_y.min() >= 0 and acc_y.max() < 2 ** 31
    for acc in (acc_u, acc_v):
        assert acc.min() >= 0 and acc.max() < limit(layout)
    return np.clip(acc_y >> SH, 0, top), np.clip(acc_u >> CSH, 0, top), np.clip(acc_v >> CSH, 0, top)


def pack(rgb, layout, chroma="center", matrix="bt601", rng="tv", m=None, off=None):
    """The bytes of one h x w x 3 frame (uint8, or float16 for a 10-bit layout) in `layout`: uint8 [frame_bytes]."""
    return write(*convert_codes(pixel_codes(rgb, layout), layout, chroma, matrix, rng, m, off), layout)


def pack_batch(frames, layout, chroma="center", matrix="bt601", rng="tv", m=None, off=None):
    return np.stack([pack(f, layout, chroma, matrix, rng, m, off) for f in frames])


def box(rgb, layout, matrix="bt601", rng="tv"):
    """What the box stage of the layout writes for a frame (the existing models)."""
    return deep_model.pack(rgb, layout, matrix, rng) if layout in DEEP else yuv_model.pack(rgb, layout, matrix, rng)


def weave_of_fields(rgb, layout, matrix="bt601", rng="tv"):
    """The existing box model run on each field as an h/2 x w frame of its own, the two results woven: luma rows f, f + 2, ... and
    chroma rows f, f + 2, ... of the frame are field f's."""
    h, w = rgb.shape[:2]
    assert h % 4 == 0
    parts = [samples(box(np.ascontiguousarray(rgb[f::2]), layout, matrix, rng), h // 2, w, layout) for f in (0, 1)]
    y, u, v = (np.empty((n,) + parts[0][k].shape[1:], dtype=np.int64) for k, n in ((0, h), (1, h // 2), (2, h // 2)))
    for f in (0, 1):
        y[f::2], u[f::2], v[f::2] = parts[f]
    return write(y, u, v, layout)


def convert_float(p, layout, chroma="center", matrix="bt601", rng="tv"):
    """The float restatement behind the per-pixel codes: ((Y, U, V) int64, the float64 values before rounding): the filtered value S / 64
    in float64, the float matrix of the layout's family, rounded half up, clamped."""
    _, off, top = tables(layout, matrix, rng)
    f = float_matrix(layout, matrix, rng)
    mean = filter_sum(p, chroma).astype(np.float64) / 64.0
    raw = (p.astype(np.float64) @ f[0] + off[0], mean @ f[1] + off[1], mean @ f[2] + off[2])
    return tuple(np.clip(np.floor(r + 0.5), 0, top).astype(np.int64) for r in raw), raw


# ---- test frames ----------------------------------------------------------------------------------------------------------------------------

def to_frame(codes, layout):
    """The RGB frame whose per-pixel codes are `codes`: uint8, or the exact halves of quarter codes."""
    codes = np.ascontiguousarray(codes, dtype=np.int64)
    return np.ascontiguousarray(deep_model.to_half(codes) if layout in DEEP else codes.astype(np.uint8))


def two_colour_frame(h, w, layout, top_codes, bottom_codes):
    """A frame whose top field is one flat colour and whose bottom field another (per-pixel codes)."""
    p = np.empty((h, w, 3), dtype=np.int64)
    p[0::2], p[1::2] = top_codes, bottom_codes
    return to_frame(p, layout)


def extreme_frame(h, w, layout, row, matrix="bt601", rng="tv", low=False):
    """The frame that drives the accumulator of matrix row `row` (1 = U, 2 = V) to its maximum — the largest code in the channels with
    positive entries, 0 in the others — or, with low, to its minimum."""
    m, _, _ = tables(layout, matrix, rng)
    top = 1020 if layout in DEEP else 255
    colour = [top if (e > 0) != low else 0 for e in m[row]]
    return to_frame(np.broadcast_to(np.array(colour, dtype=np.int64), (h, w, 3)), layout)


def boundary_matrix(layout, matrix="bt601", rng="tv"):
    """(inside, outside): the named matrix with its U row replaced by one ON the admission boundary — the largest sum of positive entries
    and the largest magnitude of negative ones the header's rule admits — and by one a step past it."""
    m, off, _ = tables(layout, matrix, rng)
    x = 64 * (1020 if layout in DEEP else 255)
    k = (off[1] << CSH) + (1 << (CSH - 1))
    p, n = (limit(layout) - 1 - k) // x, k // x
    assert k + p * x < limit(layout) <= k + (p + 1) * x and k - n * x >= 0 > k - (n + 1) * x
    inside, outside = m.copy(), m.copy()
    inside[1] = (p - 7, -n, 7)
    outside[1] = (p - 6, -n, 7)
    return inside, outside
