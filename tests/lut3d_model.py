"""The 3D LUT stage in numpy (include/crtfx_lut3d.h states the arithmetic; this file restates it and nothing else).  `table` is the uint16
[N, N, N, 3] of Cube.quantise(): quarter codes 0..1020 indexed [b][g][r][c].  `apply(frames, table)` takes uint8 frames (x = u, S = 255) or
float16 frames (x = the quarter code of resize16's quantiser, S = 1020) of shape [..., 3] and returns the same dtype and shape.
`apply_codes(x, table, S, order=...)` is the integer core on codes; `order` picks how equal fractions are ordered (the result does not
depend on it: the weight between two equal fractions is 0).  `apply_float` is the float64 restatement: exact tetrahedral interpolation of
the same table at x / S, unrounded, on the 0..1020 scale."""
import numpy as np

from tests import resize16_model

QMAX = 1020
IDENTITY_SIZES = (2, 3, 4, 5, 9, 16, 17, 18, 32, 33, 34, 35, 64, 65)
ORDERS = ("stable", "reversed", "rotated")


def quantise_cube(values):
    """rint_to_even(1020 * min(max(v, 0), 1)) in float64 -> uint16."""
    v = np.asarray(values, dtype=np.float64)
    return np.rint(1020.0 * np.minimum(np.maximum(v, 0.0), 1.0)).astype(np.uint16)


def identity_table(n):
    b, g, r = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    return quantise_cube(np.stack([r, g, b], axis=-1) / float(n - 1))


def random_table(n, seed=0):
    return np.random.default_rng([seed, n, 3]).integers(0, QMAX + 1, (n, n, n, 3), dtype=np.int64).astype(np.uint16)


def write_cube(path, values, title=""):
    """Write float64 [N, N, N, 3] ([b][g][r][c]) as a `.cube` file, red fastest, 17 significant digits: Cube.load gives the values back."""
    v = np.asarray(values, dtype=np.float64)
    with open(path, "w", encoding="utf-8") as f:
        if title:
            f.write(f'TITLE "{title}"\n')
        f.write(f"LUT_3D_SIZE {v.shape[0]}\nDOMAIN_MIN 0 0 0\nDOMAIN_MAX 1 1 1\n")
        for r, g, b in v.reshape(-1, 3).tolist():
            f.write(f"{r!r} {g!r} {b!r}\n")


def split(x, n, S):
    """codes [..., 3] -> (i, f): the cell and the fraction numerators per channel."""
    num = np.asarray(x, dtype=np.int64) * (n - 1)
    i = np.minimum(num // S, n - 2)
    return i, num - i * S


def _perm(f, order):
    """Indices [..., 3] that order the three fractions descending; ties broken three different ways."""
    if order == "stable":
        return np.argsort(-f, axis=-1, kind="stable")
    if order == "reversed":                                     # ties: the later channel first
        return 2 - np.argsort(-f[..., ::-1], axis=-1, kind="stable")
    key = -f * 4 + np.array([1, 2, 0])                          # ties: g, b, r... a rotation of the channel order
    return np.argsort(key, axis=-1, kind="stable")


def apply_codes(x, table, S, order="stable"):
    """x: integer codes 0..S, [..., 3] (r, g, b) -> int64 [..., 3]: (sum + 510) // 1020; also returns sum."""
    t = np.asarray(table).astype(np.int64)
    n = t.shape[0]
    x = np.asarray(x, dtype=np.int64)
    assert x.min(initial=0) >= 0 and x.max(initial=0) <= S and t.max() <= QMAX
    i, f = split(x, n, S)
    assert f.min(initial=0) >= 0 and f.max(initial=0) <= S
    perm = _perm(f, order)
    fs = np.take_along_axis(f, perm, axis=-1)                   # f1 >= f2 >= f3
    assert (fs[..., 0] >= fs[..., 1]).all() and (fs[..., 1] >= fs[..., 2]).all()
    eye = np.eye(3, dtype=np.int64)
    e1, e2 = eye[perm[..., 0]], eye[perm[..., 1]]               # unit steps in (r, g, b)

    def at(p):                                                  # p [..., 3] in (r, g, b) -> entries [..., 3]
        return t[p[..., 2], p[..., 1], p[..., 0]]
    w = np.stack([S - fs[..., 0], fs[..., 0] - fs[..., 1], fs[..., 1] - fs[..., 2], fs[..., 2]], axis=-1)
    assert (w >= 0).all() and (w.sum(axis=-1) == S).all()
    total = (w[..., 0, None] * at(i) + w[..., 1, None] * at(i + e1) + w[..., 2, None] * at(i + e1 + e2) + w[..., 3, None] * at(i + 1))
    assert total.max(initial=0) <= QMAX * QMAX < 2 ** 31
    return (total + 510) // 1020, total


def apply(frames, table, order="stable"):
    frames = np.asarray(frames)
    if frames.dtype == np.uint8:
        out, _ = apply_codes(frames, table, 255, order)
        assert out.max(initial=0) <= 255
        return out.astype(np.uint8)
    assert frames.dtype == np.float16
    out, _ = apply_codes(resize16_model.quantise(frames), table, QMAX, order)
    return resize16_model.to_half(out)


def apply_float(x, table, S):
    """The float64 restatement: tetrahedral interpolation of float(table) at position x * (N - 1) / S, on the table's scale."""
    t = np.asarray(table).astype(np.float64)
    n = t.shape[0]
    pos = np.asarray(x, dtype=np.float64) * (n - 1) / S
    i = np.minimum(np.floor(pos), n - 2).astype(np.int64)
    f = pos - i
    perm = np.argsort(-f, axis=-1, kind="stable")
    fs = np.take_along_axis(f, perm, axis=-1)
    eye = np.eye(3, dtype=np.int64)
    e1, e2 = eye[perm[..., 0]], eye[perm[..., 1]]

    def at(p):
        return t[p[..., 2], p[..., 1], p[..., 0]]
    return ((1.0 - fs[..., 0, None]) * at(i) + (fs[..., 0] - fs[..., 1])[..., None] * at(i + e1)
            + (fs[..., 1] - fs[..., 2])[..., None] * at(i + e1 + e2) + fs[..., 2, None] * at(i + 1))


def pixels(dtype, n_pixels, seed=0):
    """[n_pixels, 3] of `dtype`: random pixels, then grey ones (equal fractions), then pixels with one or more channels at S, the corners
    of the cube among them; for float16 random bit patterns (NaN, infinities, negatives, values above 255) and resize16's SPECIALS too."""
    rng = np.random.default_rng([seed, n_pixels, 7])
    if dtype == np.uint8:
        px = rng.integers(0, 256, (n_pixels, 3), dtype=np.int64)
        top = 255
    else:
        px = rng.integers(0, QMAX + 1, (n_pixels, 3), dtype=np.int64)
        top = QMAX
    k = n_pixels // 4
    grey = rng.integers(0, top + 1, k, dtype=np.int64)
    px[k:2 * k] = grey[:, None]                                 # grey: the three fractions are equal
    edge = rng.integers(1, 8, k, dtype=np.int64)                # bit c set: channel c at S
    for c in range(3):
        sel = np.nonzero(edge >> c & 1)[0] + 2 * k
        px[sel, c] = top
    if n_pixels >= 8:
        px[:8] = np.array([[(m >> c & 1) * top for c in range(3)] for m in range(8)])   # the eight corners
    if dtype == np.uint8:
        return px.astype(np.uint8)
    out = (px / 4.0).astype(np.float16)
    wild = rng.random(n_pixels) < 0.2                           # one sample of such a pixel is any bit pattern
    bits = out.view(np.uint16).copy()
    ch = rng.integers(0, 3, n_pixels)
    rnd = rng.integers(0, 1 << 16, n_pixels, dtype=np.int64).astype(np.uint16)
    sp = resize16_model.SPECIALS[rng.integers(0, len(resize16_model.SPECIALS), n_pixels)]
    pick = np.where(rng.random(n_pixels) < 0.5, rnd, sp)
    rows = np.nonzero(wild)[0]
    rows = rows[rows >= 8]
    bits[rows, ch[rows]] = pick[rows]
    frac = rng.random(n_pixels) < 0.2                           # ... and some carry halves between quarter codes
    rows = np.nonzero(frac & ~wild)[0]
    rows = rows[rows >= 8]
    off = (rng.random((n_pixels, 3)) * 255.0).astype(np.float16).view(np.uint16)
    bits[rows] = off[rows]
    return bits.view(np.float16)
