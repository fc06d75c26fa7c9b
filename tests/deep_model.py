"""Host model of the 10-bit pair (include/crtfx_deep.h): yuv420p10le / p010le -> half RGB and half RGB -> yuv420p10le / p010le in numpy
int64, the arithmetic written out with the eight matrices as literals (NOT imported from pythoncrt_amd.tables: tests/test_deep_tables.py
holds tables.rgb_matrix10 / yuv_matrix10 to them), plus float64 restatements that the integer models are compared with.  Packed frames are
uint8 arrays of frame_bytes bytes (little-endian 16-bit words), as the stages take and give them; `words` / `to_bytes` change the view."""
import numpy as np

SH = 16
QMAX, CMAX = 1020, 1023                 # the largest quarter code (255.0 on the half scale), the largest 10-bit code
# source: rows R, G, B over the columns (Y, U, V), 10-bit codes -> quarter codes
RGB_MATRICES = {
    ("bt601", "tv"): ((76309, 0, 104597), (76309, -25675, -53279), (76309, 132201, 0)),
    ("bt601", "pc"): ((65344, 0, 91612), (65344, -22487, -46664), (65344, 115789, 0)),
    ("bt709", "tv"): ((76309, 0, 117489), (76309, -13975, -34925), (76309, 138438, 0)),
    ("bt709", "pc"): ((65344, 0, 102903), (65344, -12240, -30589), (65344, 121252, 0)),
}
# egress: rows Y, U, V over the columns (R, G, B), quarter codes -> 10-bit codes
YUV_MATRICES = {
    ("bt601", "tv"): ((16829, 33039, 6416), (-9714, -19070, 28784), (28784, -24103, -4681)),
    ("bt601", "pc"): ((19653, 38583, 7493), (-11091, -21773, 32864), (32864, -27519, -5345)),
    ("bt709", "tv"): ((11966, 40254, 4064), (-6596, -22188, 28784), (28784, -26145, -2639)),
    ("bt709", "pc"): ((13974, 47009, 4746), (-7531, -25333, 32864), (32864, -29851, -3013)),
}
OFFSETS = {"tv": (64, 512, 512), "pc": (0, 512, 512)}
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
CASES = sorted(RGB_MATRICES)
LAYOUTS = ("yuv420p10le", "p010le")


def sizes(h, w):
    """(ch, cw, frame_bytes)"""
    ch, cw = (h + 1) // 2, (w + 1) // 2
    return ch, cw, 2 * (h * w + 2 * ch * cw)


def words(packed):
    """The uint16 words of a packed frame (uint8 [.., frame_bytes], little-endian)."""
    p = np.ascontiguousarray(packed)
    assert p.dtype == np.uint8
    return p.view("<u2")


def to_bytes(w16):
    return np.ascontiguousarray(w16, dtype="<u2").view(np.uint8)


def planes(packed, h, w, layout):
    """The SAMPLES (Y [h, w], U [ch, cw], V [ch, cw]) int64 of one packed frame: word & 1023 (yuv420p10le, Y | U | V) or word >> 6 (p010le,
    Y | interleaved U, V), rows unpadded.  The bits of a word outside its sample are ignored."""
    ch, cw, fb = sizes(h, w)
    p = words(np.asarray(packed).reshape(-1)).astype(np.int64)
    assert p.shape == (fb // 2,)
    if layout == "p010le":
        s = p >> 6
        uv = s[h * w:].reshape(ch, cw, 2)
        return s[:h * w].reshape(h, w), uv[..., 0], uv[..., 1]
    assert layout == "yuv420p10le"
    s = p & CMAX
    return s[:h * w].reshape(h, w), s[h * w:h * w + ch * cw].reshape(ch, cw), s[h * w + ch * cw:].reshape(ch, cw)


def pack_planes(y, u, v, layout):
    """The inverse of `planes` for samples 0..1023: uint8 [frame_bytes]; word = v (yuv420p10le) or v << 6 (p010le)."""
    if layout == "p010le":
        return to_bytes(np.concatenate([y.reshape(-1), np.stack([u, v], axis=2).reshape(-1)]).astype(np.int64) << 6)
    assert layout == "yuv420p10le"
    return to_bytes(np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]))


def relayout(packed420, h, w, layout):
    """A frame given as yuv420p10le, in `layout` (the same samples)."""
    return pack_planes(*planes(packed420, h, w, "yuv420p10le"), layout)


# ---- source ---------------------------------------------------------------------------------------------------------------------------------

def terms(packed, h, w, layout, rng):
    """(c, d, e) int64 [h, w] each: the samples less their offsets, chroma replicated over its 2 x 2 block (an odd edge reads the last sample)."""
    y, u, v = planes(packed, h, w, layout)
    off = OFFSETS[rng]
    yy, xx = np.arange(h) >> 1, np.arange(w) >> 1
    return y - off[0], u[yy][:, xx] - off[1], v[yy][:, xx] - off[2]


def quarter_codes(c, d, e, matrix="bt601", rng="tv"):
    """The source arithmetic on arrays of (c, d, e): quarter codes int64 [..., 3]."""
    m = np.array(RGB_MATRICES[(matrix, rng)], dtype=np.int64)
    acc = np.stack([m[k, 0] * c + m[k, 1] * d + m[k, 2] * e + (1 << (SH - 1)) for k in range(3)], axis=-1)
    assert acc.min() >= -2 ** 31 and acc.max() < 2 ** 31
    return np.clip(acc >> SH, 0, QMAX)


def to_half(q):
    """half(q / 4): exact for every quarter code (tests/test_deep_tables.py)."""
    return (np.asarray(q, dtype=np.float64) / 4.0).astype(np.float16)


def unpack(packed, h, w, layout="yuv420p10le", matrix="bt601", rng="tv"):
    """float16 [h, w, 3] RGB on the 0..255 scale of one packed frame."""
    return to_half(quarter_codes(*terms(packed, h, w, layout, rng), matrix, rng))


def rgb_float_matrix(matrix, rng):
    """The float64 inverse matrix (rows R, G, B over Y, U, V) from 10-bit codes to quarter codes."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    sy, sc = (1020.0 / 876.0, 1020.0 / 896.0) if rng == "tv" else (1020.0 / 1023.0, 1020.0 / 1023.0)
    return np.array([[sy, 0.0, 2.0 * (1.0 - kr) * sc],
                     [sy, -2.0 * kb * (1.0 - kb) / kg * sc, -2.0 * kr * (1.0 - kr) / kg * sc],
                     [sy, 2.0 * (1.0 - kb) * sc, 0.0]], dtype=np.float64)


def quarter_codes_float(c, d, e, matrix="bt601", rng="tv"):
    """The float restatement of the source: (quarter codes int64 [..., 3], the float64 values before rounding)."""
    f = rgb_float_matrix(matrix, rng)
    c, d, e = (np.asarray(x, dtype=np.float64) for x in (c, d, e))
    raw = np.stack([f[k, 0] * c + f[k, 1] * d + f[k, 2] * e for k in range(3)], axis=-1)
    return np.clip(np.floor(raw + 0.5), 0, QMAX).astype(np.int64), raw


# ---- egress ---------------------------------------------------------------------------------------------------------------------------------

def quantise(rgb_half):
    """q = rint_to_even(min(max(4 f, 0), 1020)), NaN -> 0, of float16 values: int64.  4 f is exact in float64 as it is in float32."""
    assert rgb_half.dtype == np.float16
    with np.errstate(invalid="ignore"):             # signalling NaN patterns
        t = 4.0 * rgb_half.astype(np.float64)
        t = np.where(t > 0.0, t, 0.0)               # NaN, -0, negatives, -inf -> 0
    return np.rint(np.minimum(t, float(QMAX))).astype(np.int64)


def box_sum(q):
    """S[cy][cx]: the four quarter codes under a chroma sample, the last row / column replicated at an odd edge.  int64 [ch, cw, 3]."""
    h, w = q.shape[:2]
    y0, x0 = np.arange(0, h, 2), np.arange(0, w, 2)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    return q[y0][:, x0] + q[y0][:, x1] + q[y1][:, x0] + q[y1][:, x1]


def convert_codes(q, matrix="bt601", rng="tv"):
    """(Y [h, w], U [ch, cw], V [ch, cw]) int64 10-bit codes of quarter codes int64 [h, w, 3]."""
    m, off = np.array(YUV_MATRICES[(matrix, rng)], dtype=np.int64), OFFSETS[rng]
    acc_y = q @ m[0] + (off[0] << SH) + (1 << (SH - 1))
    s = box_sum(q)
    acc_u = s @ m[1] + (off[1] << (SH + 2)) + (1 << (SH + 1))
    acc_v = s @ m[2] + (off[2] << (SH + 2)) + (1 << (SH + 1))
    for acc in (acc_y, acc_u, acc_v):
        assert acc.min() >= 0 and acc.max() < 2 ** 31
    return np.clip(acc_y >> SH, 0, CMAX), np.clip(acc_u >> (SH + 2), 0, CMAX), np.clip(acc_v >> (SH + 2), 0, CMAX)


def pack(rgb_half, layout="yuv420p10le", matrix="bt601", rng="tv"):
    """The bytes of one float16 h x w x 3 frame: uint8 [frame_bytes]."""
    return pack_planes(*convert_codes(quantise(rgb_half), matrix, rng), layout)


def yuv_float_matrix(matrix, rng):
    """The float64 matrix (rows Y, U, V) from quarter codes to 10-bit codes."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    sy, sc = (876.0 / 1020.0, 896.0 / 1020.0) if rng == "tv" else (1023.0 / 1020.0, 1023.0 / 1020.0)
    return np.array([[kr * sy, kg * sy, kb * sy],
                     [-kr / (2.0 * (1.0 - kb)) * sc, -kg / (2.0 * (1.0 - kb)) * sc, 0.5 * sc],
                     [0.5 * sc, -kg / (2.0 * (1.0 - kr)) * sc, -kb / (2.0 * (1.0 - kr)) * sc]], dtype=np.float64)


def convert_codes_float(q, matrix="bt601", rng="tv"):
    """The float restatement of the egress behind the quantiser: ((Y, U, V) int64, (y, u, v) the float64 values before rounding); chroma
    from the float mean S / 4."""
    f, off = yuv_float_matrix(matrix, rng), OFFSETS[rng]
    mean = box_sum(q).astype(np.float64) / 4.0
    raw = (q.astype(np.float64) @ f[0] + off[0], mean @ f[1] + off[1], mean @ f[2] + off[2])
    return tuple(np.clip(np.floor(r + 0.5), 0, CMAX).astype(np.int64) for r in raw), raw


# ---- test frames ----------------------------------------------------------------------------------------------------------------------------

# (Y, U, V): the clamp colours of the 8-bit source model (tests/unpack_model.py) x 4 — limited-range white with V = 960 passes 1020 in R,
# Y = 64, U = V = 64 is negative in R and B, Y = 64, U = V = 960 in G — and the 0 / 1023 corners
CLAMP_COLOURS_8 = [(235, 128, 240), (16, 16, 16), (16, 240, 240), (16, 128, 128), (235, 128, 128), (0, 0, 0), (255, 255, 255), (255, 0, 255), (0, 255, 0),
                   (255, 255, 0), (0, 0, 255), (128, 16, 240), (128, 240, 16)]
CORNERS = [(a, b, c) for a in (0, CMAX) for b in (0, CMAX) for c in (0, CMAX)]
PALETTE = [tuple(4 * x for x in col) for col in CLAMP_COLOURS_8] + [(g, 512, 512) for g in range(1024)] + CORNERS


def images(h, w, seed=0):
    """The three packed test frames of a size, uint8 [3, frame_bytes] as yuv420p10le: random 10-bit samples; a binary 0 / 1023 one; one whose
    2 x 2 blocks are colours of PALETTE.  `relayout` turns one into p010le."""
    ch, cw, fb = sizes(h, w)
    rng = np.random.default_rng(1000 * h + w + seed)
    rand = rng.integers(0, 1024, fb // 2, dtype=np.int64)
    binary = rng.integers(0, 2, fb // 2, dtype=np.int64) * CMAX
    pal = np.array(PALETTE, dtype=np.int64)
    cy, cx = np.mgrid[0:ch, 0:cw]
    idx = (cy * 37 + cx) % len(pal)                                          # 270 x 480 holds every colour
    y = pal[idx, 0][np.arange(h) >> 1][:, np.arange(w) >> 1]                 # one luma value per 2 x 2 block
    return np.stack([to_bytes(rand), to_bytes(binary), pack_planes(y, pal[idx, 1], pal[idx, 2], "yuv420p10le")])
