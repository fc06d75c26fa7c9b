"""Host model of the egress stage (include/crtfx_egress.h): RGB -> yuv420p / nv12 in numpy int64, the arithmetic written out with the four
matrices as literals (NOT imported from pythoncrt_amd.tables: tests/test_egress_tables.py holds tables.yuv_matrix to them), plus a float64
restatement — round-half-up(F . rgb + off), chroma from the float mean of the four samples — that the integer model is compared with."""
import numpy as np

SH = 16
# rows Y, U, V
MATRICES = {
    ("bt601", "tv"): ((16829, 33039, 6416), (-9714, -19070, 28784), (28784, -24103, -4681)),
    ("bt601", "pc"): ((19595, 38470, 7471), (-11058, -21710, 32768), (32768, -27439, -5329)),
    ("bt709", "tv"): ((11966, 40254, 4064), (-6596, -22188, 28784), (28784, -26145, -2639)),
    ("bt709", "pc"): ((13933, 46871, 4732), (-7509, -25259, 32768), (32768, -29763, -3005)),
}
OFFSETS = {"tv": (16, 128, 128), "pc": (0, 128, 128)}
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
CASES = sorted(MATRICES)


def sizes(h, w):
    """(ch, cw, frame_bytes)"""
    ch, cw = (h + 1) // 2, (w + 1) // 2
    return ch, cw, h * w + 2 * ch * cw


def box_sum(rgb):
    """S[cy][cx]: the four samples under a chroma sample, the last row / column replicated at an odd edge.  int64 [ch, cw, 3]."""
    h, w = rgb.shape[:2]
    y0, x0 = np.arange(0, h, 2), np.arange(0, w, 2)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    a = rgb.astype(np.int64)
    return a[y0][:, x0] + a[y0][:, x1] + a[y1][:, x0] + a[y1][:, x1]


def convert(rgb, matrix="bt601", rng="tv"):
    """(Y [h, w], U [ch, cw], V [ch, cw]) uint8 of one uint8 h x w x 3 frame."""
    m, off = np.array(MATRICES[(matrix, rng)], dtype=np.int64), OFFSETS[rng]
    a = rgb.astype(np.int64)
    acc_y = a @ m[0] + (off[0] << SH) + (1 << (SH - 1))
    s = box_sum(rgb)
    acc_u = s @ m[1] + (off[1] << (SH + 2)) + (1 << (SH + 1))
    acc_v = s @ m[2] + (off[2] << (SH + 2)) + (1 << (SH + 1))
    for acc in (acc_y, acc_u, acc_v):
        assert acc.min() >= 0 and acc.max() < 2 ** 31
    y = np.clip(acc_y >> SH, 0, 255).astype(np.uint8)
    u = np.clip(acc_u >> (SH + 2), 0, 255).astype(np.uint8)
    v = np.clip(acc_v >> (SH + 2), 0, 255).astype(np.uint8)
    return y, u, v


def pack(rgb, layout="yuv420p", matrix="bt601", rng="tv"):
    """The frame's bytes: Y | U | V (yuv420p) or Y | interleaved U, V (nv12), rows unpadded.  uint8 [frame_bytes]."""
    y, u, v = convert(rgb, matrix, rng)
    if layout == "nv12":
        return np.concatenate([y.reshape(-1), np.stack([u, v], axis=2).reshape(-1)])
    assert layout == "yuv420p"
    return np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)])


def float_matrix(matrix, rng):
    """The float64 BT.601 / BT.709 matrix (rows Y, U, V), limited range scaled by 219/255 (Y) and 224/255 (chroma)."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    sy, sc = (219.0 / 255.0, 224.0 / 255.0) if rng == "tv" else (1.0, 1.0)
    return np.array([[kr * sy, kg * sy, kb * sy],
                     [-kr / (2.0 * (1.0 - kb)) * sc, -kg / (2.0 * (1.0 - kb)) * sc, 0.5 * sc],
                     [0.5 * sc, -kg / (2.0 * (1.0 - kr)) * sc, -kb / (2.0 * (1.0 - kr)) * sc]], dtype=np.float64)


def convert_float(rgb, matrix="bt601", rng="tv"):
    """The float restatement: ((Y, U, V) uint8, (y, u, v) the float64 values before rounding)."""
    f, off = float_matrix(matrix, rng), OFFSETS[rng]
    mean = box_sum(rgb).astype(np.float64) / 4.0
    raw = (rgb.astype(np.float64) @ f[0] + off[0], mean @ f[1] + off[1], mean @ f[2] + off[2])
    return tuple(np.clip(np.floor(r + 0.5), 0, 255).astype(np.uint8) for r in raw), raw


# pure blue / pure red reach 256 before the clamp at full range; with black, white and the other corners
CLAMP_COLOURS = [(0, 0, 255), (255, 0, 0), (0, 0, 0), (255, 255, 255), (0, 255, 0), (255, 255, 0), (0, 255, 255), (255, 0, 255)]


def images(h, w, seed=0):
    """The three test frames of a size, uint8 [3, h, w, 3]: random bytes; a binary 0 / 255 one; one that holds the clamp colours and the greys
    (CLAMP_COLOURS + the 256 greys)."""
    rng = np.random.default_rng(1000 * h + w + seed)
    rand = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    binary = (rng.integers(0, 2, (h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)
    pal = np.array(CLAMP_COLOURS + [(g, g, g) for g in range(256)], dtype=np.uint8)
    # 2 x 2 blocks of one colour (chroma = the per-pixel formula, clamp included), every seventh column shifted to the next colour (mixed blocks)
    yy, xx = np.mgrid[0:h, 0:w]
    idx = ((yy // 2) * 5 + xx // 2 + (xx % 7 == 3)) % len(pal)
    return np.stack([rand, binary, pal[idx]])
