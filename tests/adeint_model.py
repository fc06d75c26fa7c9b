"""Integer numpy model of the motion-adaptive deinterlace stage, written from include/crtfx_adeint.h on deint_model's codes / from_codes /
directions: uint8 and half frames, TFF and BFF, FIRST and BOTH, a previous frame or none.  Vectorised over the batch axis: frame i's
previous frame is frame i - 1, frame 0's is `prev`.  `adaptive_parts` also returns, per output frame, EDGE's codes e, the source's own
codes c and m on the made rows (m = -1 where the frame has no previous frame)."""
import numpy as np

from tests import deint_model as dm

ORDERS, FIELDS = dm.ORDERS, dm.FIELDS


def made_rows(h, field):
    """(ys, the row above or the one neighbour, the row below or the one neighbour) of the rows made for `field`."""
    ys = np.arange(1 - field, h, 2)
    return ys, np.where(ys > 0, ys - 1, ys + 1), np.where(ys < h - 1, ys + 1, ys - 1)


def edge_codes(c, ya, yb):
    """EDGE's codes on the made rows: c [n, h, w, 3] codes -> [n, rows, w, 3].  A row with one neighbour has a == b: S(0) = 0, d = 0 and
    (a + a + 1) >> 1 = a, the copy."""
    a, b = c[:, ya], c[:, yb]
    d = dm.directions(a, b)
    d = np.where((ya == yb)[None, :, None], 0, d)
    x = np.arange(c.shape[2])[None, None, :]
    ea = np.take_along_axis(a, np.broadcast_to((x + d)[..., None], a.shape), axis=2)
    eb = np.take_along_axis(b, np.broadcast_to((x - d)[..., None], b.shape), axis=2)
    return (ea + eb + 1) >> 1


def adaptive_parts(frames, prev=None, order="tff", fields="first"):
    frames = np.asarray(frames)
    assert frames.ndim == 4 and frames.shape[3] == 3 and frames.shape[1] >= 2 and order in ORDERS and fields in FIELDS
    n, h, w = frames.shape[:3]
    first = ORDERS.index(order)
    which = (first,) if fields == "first" else (first, 1 - first)
    per = len(which)
    out = np.repeat(frames, per, axis=0)                    # kept rows: the source's bits
    parts = [None] * per
    if n == 0:
        return out, parts
    c = dm.codes(frames)
    if prev is not None:
        prev = np.asarray(prev)
        assert prev.shape == frames.shape[1:] and prev.dtype == frames.dtype
    has_p = np.ones(n, dtype=bool)
    has_p[0] = prev is not None
    p = dm.codes(np.concatenate([(prev if prev is not None else frames[0])[None], frames[:-1]]))
    diff = np.abs(c - p)
    for j, field in enumerate(which):
        ys, ya, yb = made_rows(h, field)
        e = edge_codes(c, ya, yb)
        t0 = diff[:, ys].max(axis=-1)
        t1 = ((diff[:, ya] + diff[:, yb] + 1) >> 1).max(axis=-1)
        m = np.maximum(t0, t1)[..., None]
        cy = c[:, ys]
        r = np.minimum(np.maximum(e, cy - m), cy + m)
        r = np.where(has_p[:, None, None, None], r, e)
        out[j::per][:, ys] = dm.from_codes(r, frames.dtype.type)
        parts[j] = (e, cy, np.where(has_p[:, None, None], m[..., 0], -1), ys)
    return out, parts


def adaptive(frames, prev=None, order="tff", fields="first"):
    """frames [n, h, w, 3] uint8 or float16, prev [h, w, 3] or None -> [n * frames_out, h, w, 3] of the same dtype."""
    return adaptive_parts(frames, prev, order, fields)[0]


def clamp_classes(parts):
    """Which of {the weave (m = 0), held between (0 < m < |e - c|), EDGE's (m >= |e - c|, m > 0)} occur on the made samples."""
    seen = set()
    for e, c, m, _ in parts:
        m3, gap = np.broadcast_to(m[..., None], e.shape), np.abs(e - c)
        has = m3 >= 0
        seen |= {name for name, mask in (("weave", m3 == 0), ("held", (m3 > 0) & (m3 < gap)), ("edge", (m3 > 0) & (m3 >= gap))) if (mask & has).any()}
    return seen


def scene(n, h, w, dtype=np.uint8, seed=1, still=0.5):
    """Frames that mix still and changed regions: every frame (and a `prev` in front, returned second) is the one before it with a share
    1 - `still` of its pixels redrawn — some by a little, some wholly — so that m = 0, m below |e - c| and m above it all occur."""
    rng = np.random.default_rng(seed)
    seq = [dm.noise(h, w, 1, dtype, seed=int(rng.integers(1 << 30)))[0]]
    for _ in range(n):
        f = seq[-1].copy()
        fresh = dm.noise(h, w, 1, dtype, seed=int(rng.integers(1 << 30)))[0]
        u = rng.random((h, w))
        big = u < (1 - still) / 2
        small = (u >= (1 - still) / 2) & (u < 1 - still)
        f[big] = fresh[big]
        step = dm.codes(f) + rng.integers(-24, 25, f.shape)
        lim = 255 if dtype == np.uint8 else dm.QMAX
        f[small] = dm.from_codes(np.clip(step, 0, lim), np.dtype(dtype).type)[small]
        seq.append(f)
    return np.stack(seq[1:]), seq[0]
