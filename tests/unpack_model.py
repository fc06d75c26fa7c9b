"""Host model of the source stage (include/crtfx_unpack.h): yuv420p / nv12 -> RGB in numpy int64, the arithmetic written out with the four
matrices as literals (NOT imported from pythoncrt_amd.tables: tests/test_unpack_tables.py holds tables.rgb_matrix to them), plus a float64
restatement — round-half-up(F . (c, d, e)), clamped — that the integer model is compared with."""
import numpy as np

SH = 16
# rows R, G, B over the columns (Y, U, V)
MATRICES = {
    ("bt601", "tv"): ((76309, 0, 104597), (76309, -25675, -53279), (76309, 132201, 0)),
    ("bt601", "pc"): ((65536, 0, 91881), (65536, -22553, -46802), (65536, 116130, 0)),
    ("bt709", "tv"): ((76309, 0, 117489), (76309, -13975, -34925), (76309, 138438, 0)),
    ("bt709", "pc"): ((65536, 0, 103206), (65536, -12276, -30679), (65536, 121609, 0)),
}
OFFSETS = {"tv": (16, 128, 128), "pc": (0, 128, 128)}
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
CASES = sorted(MATRICES)


def sizes(h, w):
    """(ch, cw, frame_bytes)"""
    ch, cw = (h + 1) // 2, (w + 1) // 2
    return ch, cw, h * w + 2 * ch * cw


def planes(packed, h, w, layout):
    """(Y [h, w], U [ch, cw], V [ch, cw]) of one packed frame: Y | U | V (yuv420p) or Y | interleaved U, V (nv12), rows unpadded."""
    ch, cw, fb = sizes(h, w)
    p = np.asarray(packed).reshape(-1)
    assert p.shape == (fb,) and p.dtype == np.uint8
    y = p[:h * w].reshape(h, w)
    if layout == "nv12":
        uv = p[h * w:].reshape(ch, cw, 2)
        return y, uv[..., 0], uv[..., 1]
    assert layout == "yuv420p"
    return y, p[h * w:h * w + ch * cw].reshape(ch, cw), p[h * w + ch * cw:].reshape(ch, cw)


def pack_planes(y, u, v, layout):
    """The inverse of `planes`: uint8 [frame_bytes]."""
    if layout == "nv12":
        return np.concatenate([y.reshape(-1), np.stack([u, v], axis=2).reshape(-1)]).astype(np.uint8)
    assert layout == "yuv420p"
    return np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]).astype(np.uint8)


def terms(packed, h, w, layout, rng):
    """(c, d, e) int64 [h, w] each: the samples less their offsets, chroma replicated over its 2 x 2 block (an odd edge reads the last sample)."""
    y, u, v = planes(packed, h, w, layout)
    off = OFFSETS[rng]
    yy, xx = np.arange(h) >> 1, np.arange(w) >> 1
    return (y.astype(np.int64) - off[0], u.astype(np.int64)[yy][:, xx] - off[1], v.astype(np.int64)[yy][:, xx] - off[2])


def convert_yuv(c, d, e, matrix="bt601", rng="tv"):
    """The arithmetic on arrays of (c, d, e): uint8 [..., 3]."""
    m = np.array(MATRICES[(matrix, rng)], dtype=np.int64)
    acc = np.stack([m[k, 0] * c + m[k, 1] * d + m[k, 2] * e + (1 << (SH - 1)) for k in range(3)], axis=-1)
    assert acc.min() >= -2 ** 31 and acc.max() < 2 ** 31
    return np.clip(acc >> SH, 0, 255).astype(np.uint8)


def unpack(packed, h, w, layout="yuv420p", matrix="bt601", rng="tv"):
    """uint8 [h, w, 3] RGB of one packed uint8 frame."""
    return convert_yuv(*terms(packed, h, w, layout, rng), matrix, rng)


def float_matrix(matrix, rng):
    """The float64 BT.601 / BT.709 inverse matrix (rows R, G, B over Y, U, V), limited range scaled by 255/219 (Y) and 255/224 (chroma)."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    sy, sc = (255.0 / 219.0, 255.0 / 224.0) if rng == "tv" else (1.0, 1.0)
    return np.array([[sy, 0.0, 2.0 * (1.0 - kr) * sc],
                     [sy, -2.0 * kb * (1.0 - kb) / kg * sc, -2.0 * kr * (1.0 - kr) / kg * sc],
                     [sy, 2.0 * (1.0 - kb) * sc, 0.0]], dtype=np.float64)


def convert_yuv_float(c, d, e, matrix="bt601", rng="tv"):
    """The float restatement: (uint8 [..., 3], the float64 values before rounding)."""
    f = float_matrix(matrix, rng)
    raw = np.stack([f[k, 0] * c + f[k, 1] * d + f[k, 2] * e for k in range(3)], axis=-1)
    return np.clip(np.floor(raw + 0.5), 0, 255).astype(np.uint8), raw


def unpack_float(packed, h, w, layout="yuv420p", matrix="bt601", rng="tv"):
    c, d, e = terms(packed, h, w, layout, rng)
    return convert_yuv_float(c.astype(np.float64), d.astype(np.float64), e.astype(np.float64), matrix, rng)


# (Y, U, V): limited-range white with V = 240 exceeds 255 in R; Y = 16, U = V = 16 is negative in R and B, Y = 16, U = V = 240 in G; with black,
# white and the chroma corners
CLAMP_COLOURS = [(235, 128, 240), (16, 16, 16), (16, 240, 240), (16, 128, 128), (235, 128, 128), (0, 0, 0), (255, 255, 255), (255, 0, 255), (0, 255, 0),
                 (255, 255, 0), (0, 0, 255), (128, 16, 240), (128, 240, 16)]


def images(h, w, seed=0):
    """The three packed test frames of a size, uint8 [3, frame_bytes] in the yuv420p layout's plane order: random bytes; a binary 0 / 255
    one; one whose 2 x 2 blocks are colours of a palette (CLAMP_COLOURS + the 256 greys).  `relayout` turns one into nv12."""
    ch, cw, fb = sizes(h, w)
    rng = np.random.default_rng(1000 * h + w + seed)
    rand = rng.integers(0, 256, fb, dtype=np.uint8)
    binary = (rng.integers(0, 2, fb, dtype=np.uint8) * 255).astype(np.uint8)
    pal = np.array(CLAMP_COLOURS + [(g, 128, 128) for g in range(256)], dtype=np.uint8)
    cy, cx = np.mgrid[0:ch, 0:cw]
    idx = (cy * 5 + cx) % len(pal)
    y = pal[idx, 0][np.arange(h) >> 1][:, np.arange(w) >> 1]                 # one luma value per 2 x 2 block
    return np.stack([rand, binary, pack_planes(y, pal[idx, 1], pal[idx, 2], "yuv420p")])


def relayout(packed420p, h, w, layout):
    """A frame given in the yuv420p layout, in `layout` (the same samples)."""
    return pack_planes(*planes(packed420p, h, w, "yuv420p"), layout)
