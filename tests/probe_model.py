"""Integer numpy model of the source probe, written from include/crtfx_probe.h: uint8 and half frames -> uint32 records.  `records` is the
whole rule; `luma`, `codes` and `words` are its parts; `scene` and `boxed` build the streams the tests probe: a field-rate scene with a moving
block, woven either way round or left progressive or still, and a letterboxed / pillarboxed version of any stream with noise in the bars.
Everything is int64 until the record is packed."""
import numpy as np

from tests import deint_model as dm

QMAX = 1020
W_FLAGS, W_MIN, W_MAX, W_SUM, W_CUR, W_EVEN, W_ODD, W_HIST, W_ROWS = 0, 1, 4, 8, 10, 12, 14, 16, 272


def words(h, w):
    """uint32 words of one record: 272 + h + w rounded up to even."""
    return (W_ROWS + h + w + 1) & ~1


def codes(frame):
    """Quarter codes 0..1020: 4 u of a uint8 sample, the family's quantiser of a half sample."""
    frame = np.asarray(frame)
    return frame.astype(np.int64) * 4 if frame.dtype == np.uint8 else dm.quantise(frame)


def luma(frame):
    """Y [h, w] of a frame [h, w, 3]: (54 r + 183 g + 19 b + 128) >> 8 on codes."""
    c = codes(frame)
    return (54 * c[..., 0] + 183 * c[..., 1] + 19 * c[..., 2] + 128) >> 8


def _put64(rec, at, v):
    v = int(v)
    assert 0 <= v < 1 << 64
    rec[at], rec[at + 1] = v & 0xffffffff, v >> 32


def record(frame, prev=None):
    """The record of one frame [h, w, 3]; prev: the frame in front of it, or None."""
    frame = np.asarray(frame)
    h, w = frame.shape[:2]
    c, Y = codes(frame), luma(frame)
    rec = np.zeros(words(h, w), dtype=np.int64)
    rec[W_FLAGS] = 0 if prev is None else 1
    rec[W_MIN:W_MIN + 3] = c.reshape(-1, 3).min(axis=0)
    rec[W_MAX:W_MAX + 3] = c.reshape(-1, 3).max(axis=0)
    _put64(rec, W_SUM, Y.sum())
    if h >= 3:
        comb = Y[:-2] + Y[2:]                                                  # row y - 1 + row y + 1 at y = 1..h-2
        _put64(rec, W_CUR, np.abs(comb - 2 * Y[1:-1]).sum())
        if prev is not None:
            d = np.abs(comb - 2 * luma(prev)[1:-1]).sum(axis=1)                # per row y = 1..h-2
            ys = np.arange(1, h - 1)
            _put64(rec, W_EVEN, d[ys % 2 == 0].sum())
            _put64(rec, W_ODD, d[ys % 2 == 1].sum())
    rec[W_HIST:W_HIST + 256] = np.bincount((Y >> 2).reshape(-1), minlength=256)
    rec[W_ROWS:W_ROWS + h] = Y.sum(axis=1)
    rec[W_ROWS + h:W_ROWS + h + w] = Y.sum(axis=0)
    assert rec.min() >= 0 and rec.max() < 1 << 32
    return rec.astype(np.uint32)


def records(frames, prev=None):
    """frames [n, h, w, 3] uint8 or float16 -> uint32 [n, words]; the previous frame of frame i > 0 is frame i - 1, that of frame 0 `prev`."""
    frames = np.asarray(frames)
    n, h, w = frames.shape[:3]
    out = np.zeros((n, words(h, w)), dtype=np.uint32)
    for i in range(n):
        out[i] = record(frames[i], prev if i == 0 else frames[i - 1])
    return out


def get64(rec, at):
    return int(rec[at]) | int(rec[at + 1]) << 32


def sums(recs):
    """(S_cur, S_even, S_odd) summed over the records that had a previous frame."""
    had = [r for r in recs if int(r[W_FLAGS]) & 1]
    return tuple(sum(get64(r, at) for r in had) for at in (W_CUR, W_EVEN, W_ODD))


# ---- scenes --------------------------------------------------------------------------------------------------------------------------------

KINDS = ("tff", "bff", "progressive", "still")


def scene(kind, n=6, h=24, w=40, dtype=np.uint8, seed=3, step=1):
    """n frames [n, h, w, 3]: vertical grey stripes of smooth texture, every row the same, that move `step` pixels per FIELD time (they wrap).  "tff" /
    "bff": one picture per field, woven two to a frame with that field first; "progressive": one picture per frame (the block moves 2 step per frame);
    "still": the block does not move."""
    assert kind in KINDS
    rng = np.random.default_rng(seed)
    u = np.arange(w)
    tri = 30 + 24 * np.abs(u % 16 - 8)                                         # a triangle wave: what a pixel changes by grows with the distance moved
    band = np.stack([tri, tri, tri], axis=-1) + rng.integers(0, 2, (w, 3))      # grey, so that a 4:2:0 format's chroma rows, which pair the two fields, carry nothing

    def picture(t):                                                            # t in field times
        return np.broadcast_to(np.roll(band, 0 if kind == "still" else step * t, axis=0)[None], (h, w, 3))
    out = np.empty((n, h, w, 3), dtype=np.int64)
    for i in range(n):
        if kind in ("tff", "bff"):
            first = KINDS.index(kind)                                          # the parity of the rows the first field fills
            out[i, first::2] = picture(2 * i)[first::2]
            out[i, 1 - first::2] = picture(2 * i + 1)[1 - first::2]
        else:
            out[i] = picture(2 * i)
    out = np.clip(out, 0, 255)
    return out.astype(np.uint8) if dtype == np.uint8 else out.astype(np.float16)


def boxed(frames, full, at, noise=5, seed=11):
    """`frames` [n, ph, pw, 3] placed at `at` = (y, x) on frames of `full` = (h, w) whose bars hold noise of 0..noise (of 255): a letterboxed
    or pillarboxed stream.  The picture is lifted to at least 40 so that every one of its rows and columns is above any sensible limit."""
    frames = np.asarray(frames)
    n, ph, pw = frames.shape[:3]
    rng = np.random.default_rng(seed)
    out = rng.integers(0, noise + 1, (n,) + tuple(full) + (3,)).astype(frames.dtype)
    pic = np.maximum(frames, np.asarray(40, dtype=frames.dtype))
    out[:, at[0]:at[0] + ph, at[1]:at[1] + pw] = pic
    return out
