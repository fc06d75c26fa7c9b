"""Integer numpy model of the deinterlace stage, written from include/crtfx_deint.h: uint8 and half frames, LINEAR and EDGE, TFF and BFF,
FIRST and BOTH.  `deinterlace` returns the output frames; `deinterlace_d` returns the directions taken as well.  Everything is int64; kept
rows are moved as bits."""
import numpy as np

METHODS = ("linear", "edge")
ORDERS = ("tff", "bff")
FIELDS = ("first", "both")
QMAX = 1020
REACH = 3                           # the search of a pixel reaches columns x - 3 .. x + 3
STEPS = (-1, 1)                     # the order in which the two sides are tried


def quantise(half):
    """q = rint_to_even(min(max(4 f, 0), 1020)), NaN -> 0, of float16 values, as int64."""
    half = np.asarray(half)
    assert half.dtype == np.float16
    with np.errstate(invalid="ignore"):
        t = 4.0 * half.astype(np.float64)           # exact
        t = np.where(t > 0.0, t, 0.0)               # NaN, -0, negatives, -inf -> 0
    return np.rint(np.minimum(t, float(QMAX))).astype(np.int64)


def codes(frame):
    """The integers the arithmetic runs on: 0..255 of a uint8 frame, quarter codes 0..1020 of a half frame."""
    frame = np.asarray(frame)
    if frame.dtype == np.uint8:
        return frame.astype(np.int64)
    return quantise(frame)


def from_codes(c, dtype):
    """A result as a sample: the code itself for uint8, half(c / 4) — exact — for half."""
    if dtype == np.uint8:
        assert c.min() >= 0 and c.max() <= 255
        return c.astype(np.uint8)
    assert c.min() >= 0 and c.max() <= QMAX
    out = (c.astype(np.float64) / 4.0).astype(np.float16)
    assert np.array_equal(out.astype(np.float64) * 4.0, c)
    return out


def _shift(rows, j):
    """rows[..., x + j, :] at every x, zero where x + j leaves the row (those columns are never used: the caller masks them)."""
    out = np.zeros_like(rows)
    w = rows.shape[-2]
    if abs(j) >= w:
        return out
    if j >= 0:
        out[..., :w - j, :] = rows[..., j:, :]
    else:
        out[..., -j:, :] = rows[..., :w + j, :]
    return out


def score(a, b, j):
    """S(j) at every column of rows a, b [..., w, 3]: sum over t in {-1, 0, 1} and the three channels of |a[x + t + j] - b[x + t - j]|;
    meaningful where REACH <= x <= w - 1 - REACH."""
    s = np.zeros(a.shape[:-1], dtype=np.int64)
    for t in (-1, 0, 1):
        s += np.abs(_shift(a, t + j) - _shift(b, t - j)).sum(axis=-1)
    return s


def directions(a, b):
    """The direction d of every pixel of the rows between the kept rows a and b (int64 [..., w, 3] codes): 0 where x < 3 or x > w - 4."""
    w = a.shape[-2]
    d = np.zeros(a.shape[:-1], dtype=np.int64)
    x = np.arange(w)
    inner = (x >= REACH) & (x <= w - 1 - REACH)
    if not inner.any() or a.size == 0:
        return d
    s0 = score(a, b, 0)
    assert s0[..., inner].max() <= 9 * QMAX
    s = s0 - 1
    for j in STEPS:
        s1 = score(a, b, j)
        take = inner & (s1 < s)
        s = np.where(take, s1, s)
        d = np.where(take, j, d)
        s2 = score(a, b, 2 * j)
        take2 = take & (s2 < s)                     # the second step only behind a successful first one
        s = np.where(take2, s2, s)
        d = np.where(take2, 2 * j, d)
    return d


def field_frame(frame, field, method):
    """The progressive frame made for `field` (0: the even rows are kept, 1: the odd rows) of one h x w x 3 frame, and the directions
    [h, w] (0 on kept rows)."""
    frame = np.asarray(frame)
    h, w = frame.shape[:2]
    assert h >= 2 and frame.shape[2] == 3 and method in METHODS and field in (0, 1)
    c = codes(frame)
    out = frame.copy()                              # kept rows: the source's bits
    dirs = np.zeros((h, w), dtype=np.int64)
    missing = np.arange(1 - field, h, 2)
    for y in missing[(missing == 0) | (missing == h - 1)]:      # one neighbour in the frame: a copy of it
        out[y] = from_codes(c[1] if y == 0 else c[h - 2], frame.dtype.type)
    ys = missing[(missing > 0) & (missing < h - 1)]
    if ys.size:
        a, b = c[ys - 1], c[ys + 1]
        d = directions(a, b) if method == "edge" else np.zeros((ys.size, w), dtype=np.int64)
        x = np.arange(w)[None, :]
        r = np.arange(ys.size)[:, None]
        out[ys] = from_codes((a[r, x + d] + b[r, x - d] + 1) >> 1, frame.dtype.type)
        dirs[ys] = d
    return out, dirs


def deinterlace_d(frames, method="linear", order="tff", fields="first"):
    """frames [n, h, w, 3] uint8 or float16 -> (out [n * frames_out, h, w, 3] of the same dtype, directions [n * frames_out, h, w])."""
    frames = np.asarray(frames)
    assert frames.ndim == 4 and order in ORDERS and fields in FIELDS
    first = ORDERS.index(order)
    outs, dirs = [], []
    for f in frames:
        for field in ((first,) if fields == "first" else (first, 1 - first)):
            o, d = field_frame(f, field, method)
            outs.append(o)
            dirs.append(d)
    shape = (0,) + frames.shape[1:]
    return (np.stack(outs) if outs else np.zeros(shape, frames.dtype)), (np.stack(dirs) if dirs else np.zeros(shape[:3], np.int64))


def deinterlace(frames, method="linear", order="tff", fields="first"):
    return deinterlace_d(frames, method, order, fields)[0]


def bits(a):
    """The samples as unsigned integers, so that NaN payloads compare."""
    a = np.asarray(a)
    return a.view(np.uint16) if a.dtype == np.float16 else a


def noise(h, w, n=1, dtype=np.uint8, seed=5):
    """Seeded uniform noise: bytes, or quarter codes as halves."""
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    return (rng.integers(0, QMAX + 1, (n, h, w, 3)).astype(np.float64) / 4.0).astype(np.float16)


def stripes(h, w, slope, dtype=np.uint8):
    """A frame of straight stripes on a ramp: the picture at (y, x) is step * (x + slope * y) + const, so that between rows y - 1 and
    y + 1 the pair a[x + j], b[x - j] differs by 2 * step * |j - slope| in the first channel: S(j) is 0 at j = slope and grows with
    |j - slope|, and the search walks to d = slope.  w - 1 + |slope| * (h - 1) <= 42 keeps the ramp inside 0..255."""
    y, x = np.mgrid[0:h, 0:w]
    u = x + slope * y
    u = u - u.min()
    assert u.max() <= 42
    v = 6 * u
    f = np.stack([v, 255 - v, v // 2], axis=-1)
    return f.astype(np.uint8)[None] if dtype == np.uint8 else f.astype(np.float16)[None]
