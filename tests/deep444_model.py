"""Host model of the 10-bit 4:4:4 pair (include/crtfx_444.h): yuv444p10le / gbrp10le / x2rgb10le -> half RGB and back in numpy int64, the
arithmetic written out with every matrix as a literal (NOT imported from pythoncrt_amd.tables: tests/test_deep444_tables.py holds
tables.rgb_matrix10 / yuv_matrix10 / rgb_scale10 to them), plus the float64 restatements the integer models are compared with.  Packed
frames are uint8 arrays of frame_bytes bytes (little-endian 16-bit or 32-bit words), as the stages take and give them."""
import numpy as np

SH = 16
QMAX, CMAX = 1020, 1023                 # the largest quarter code (255.0 on the half scale), the largest 10-bit code
K_IN, K_OUT = 65344, 65729              # floor(1020/1023 * 65536 + 0.5), floor(1023/1020 * 65536 + 0.5)
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
# the two full-range RGB formats: source rows R, G, B over the planes / fields; egress rows = planes / fields over R, G, B; offsets 0
SCALE_IN = {"gbr": ((0, 0, K_IN), (K_IN, 0, 0), (0, K_IN, 0)), "rgb": ((K_IN, 0, 0), (0, K_IN, 0), (0, 0, K_IN))}
SCALE_OUT = {"gbr": ((0, K_OUT, 0), (0, 0, K_OUT), (K_OUT, 0, 0)), "rgb": ((K_OUT, 0, 0), (0, K_OUT, 0), (0, 0, K_OUT))}
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
CASES = sorted(RGB_MATRICES)
FORMATS = ("yuv444p10le", "gbrp10le", "x2rgb10le")
ORDER = {"gbrp10le": "gbr", "x2rgb10le": "rgb"}


def source_table(fmt, matrix="bt601", rng="tv"):
    """(m int64 [3, 3], off int64 [3]) of the source stage; `matrix` and `rng` apply to yuv444p10le only."""
    if fmt in ORDER:
        return np.array(SCALE_IN[ORDER[fmt]], dtype=np.int64), np.zeros(3, dtype=np.int64)
    assert fmt == "yuv444p10le"
    return np.array(RGB_MATRICES[(matrix, rng)], dtype=np.int64), np.array(OFFSETS[rng], dtype=np.int64)


def egress_table(fmt, matrix="bt601", rng="tv"):
    if fmt in ORDER:
        return np.array(SCALE_OUT[ORDER[fmt]], dtype=np.int64), np.zeros(3, dtype=np.int64)
    assert fmt == "yuv444p10le"
    return np.array(YUV_MATRICES[(matrix, rng)], dtype=np.int64), np.array(OFFSETS[rng], dtype=np.int64)


def sizes(h, w, fmt):
    """frame_bytes"""
    assert fmt in FORMATS
    return h * w * (4 if fmt == "x2rgb10le" else 6)


def samples(packed, h, w, fmt):
    """The SAMPLES P int64 [3, h, w] of one packed frame: word & 1023 of plane j (planar), or the three 10-bit fields of a 32-bit word from
    the top down (x2rgb10le).  The bits outside a sample are ignored."""
    p = np.ascontiguousarray(np.asarray(packed).reshape(-1))
    assert p.dtype == np.uint8 and p.size == sizes(h, w, fmt)
    if fmt == "x2rgb10le":
        d = p.view("<u4").astype(np.int64).reshape(h, w)
        return np.stack([(d >> 20) & CMAX, (d >> 10) & CMAX, d & CMAX])
    return (p.view("<u2").astype(np.int64) & CMAX).reshape(3, h, w)


def pack_samples(P, fmt):
    """The inverse of `samples` for samples 0..1023 (int64 [3, h, w]): uint8 [frame_bytes], the bits outside a sample 0."""
    P = np.asarray(P, dtype=np.int64)
    assert P.min() >= 0 and P.max() <= CMAX
    if fmt == "x2rgb10le":
        return np.ascontiguousarray(((P[0] << 20) | (P[1] << 10) | P[2]).reshape(-1), dtype="<u4").view(np.uint8)
    assert fmt in FORMATS
    return np.ascontiguousarray(P.reshape(-1), dtype="<u2").view(np.uint8)


def relayout(planar, h, w, fmt):
    """A frame given in the planar layout, in the layout of `fmt` (the same samples P0, P1, P2)."""
    return pack_samples(samples(planar, h, w, "yuv444p10le"), fmt)


# ---- source ----

def quarter_codes(P, m, off):
    """The source arithmetic on samples int64 [3, ...]: quarter codes int64 [..., 3]."""
    c = [P[j] - off[j] for j in range(3)]
    acc = np.stack([m[k, 0] * c[0] + m[k, 1] * c[1] + m[k, 2] * c[2] + (1 << (SH - 1)) for k in range(3)], axis=-1)
    assert acc.min() >= -2 ** 31 and acc.max() < 2 ** 31
    return np.clip(acc >> SH, 0, QMAX)


def to_half(q):
    """half(q / 4): exact for every quarter code."""
    return (np.asarray(q, dtype=np.float64) / 4.0).astype(np.float16)


def unpack(packed, h, w, fmt="yuv444p10le", matrix="bt601", rng="tv"):
    """float16 [h, w, 3] RGB on the 0..255 scale of one packed frame."""
    return to_half(quarter_codes(samples(packed, h, w, fmt), *source_table(fmt, matrix, rng)))


def source_float_matrix(fmt, matrix="bt601", rng="tv"):
    """The float64 matrix of the source (rows R, G, B over P0, P1, P2), 10-bit codes to quarter codes, nothing rounded."""
    if fmt in ORDER:
        return np.array(SCALE_IN[ORDER[fmt]], dtype=np.float64) / K_IN * (1020.0 / 1023.0)
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    sy, sc = (1020.0 / 876.0, 1020.0 / 896.0) if rng == "tv" else (1020.0 / 1023.0, 1020.0 / 1023.0)
    return np.array([[sy, 0.0, 2.0 * (1.0 - kr) * sc],
                     [sy, -2.0 * kb * (1.0 - kb) / kg * sc, -2.0 * kr * (1.0 - kr) / kg * sc],
                     [sy, 2.0 * (1.0 - kb) * sc, 0.0]], dtype=np.float64)


def quarter_codes_float(P, fmt, matrix="bt601", rng="tv"):
    """The float restatement of the source: (quarter codes int64 [..., 3], the float64 values before rounding)."""
    f, off = source_float_matrix(fmt, matrix, rng), source_table(fmt, matrix, rng)[1]
    c = [np.asarray(P[j], dtype=np.float64) - float(off[j]) for j in range(3)]
    raw = np.stack([f[k, 0] * c[0] + f[k, 1] * c[1] + f[k, 2] * c[2] for k in range(3)], axis=-1)
    return np.clip(np.floor(raw + 0.5), 0, QMAX).astype(np.int64), raw


# ---- egress ----

def quantise(rgb_half):
    """q = rint_to_even(min(max(4 f, 0), 1020)), NaN -> 0, of float16 values: int64.  4 f is exact in float64 as it is in float32."""
    assert rgb_half.dtype == np.float16
    with np.errstate(invalid="ignore"):             # signalling NaN patterns
        t = 4.0 * rgb_half.astype(np.float64)
        t = np.where(t > 0.0, t, 0.0)               # NaN, -0, negatives, -inf -> 0
    return np.rint(np.minimum(t, float(QMAX))).astype(np.int64)


def accumulators(q, m, off):
    """The three egress accumulators int64 [3, ...] of quarter codes int64 [..., 3]."""
    return np.stack([q @ m[j] + (int(off[j]) << SH) + (1 << (SH - 1)) for j in range(3)])


def convert_codes(q, m, off):
    """The samples T int64 [3, ...] of quarter codes int64 [..., 3]."""
    acc = accumulators(q, m, off)
    assert acc.min() >= 0 and acc.max() < 2 ** 31
    return np.clip(acc >> SH, 0, CMAX)


def convert_codes_float(q, m, off):
    """The float64 restatement of the egress with the SAME integer matrix: floor(m . q / 65536 + off + 0.5), clamped."""
    raw = np.stack([(q.astype(np.float64) @ m[j].astype(np.float64)) / 65536.0 + float(off[j]) for j in range(3)])
    return np.clip(np.floor(raw + 0.5), 0, CMAX).astype(np.int64)


def pack(rgb_half, fmt="yuv444p10le", matrix="bt601", rng="tv"):
    """The bytes of one float16 h x w x 3 frame: uint8 [frame_bytes]."""
    return pack_samples(convert_codes(quantise(rgb_half), *egress_table(fmt, matrix, rng)), fmt)


# ---- test frames ----

# (P0, P1, P2): the clamp colours of the 10-bit 4:2:0 model (as Y, U, V: limited-range white with V = 960 passes 1020 in R, Y = 64 with
# U = V = 64 is negative in R and B, with U = V = 960 in G), every grey, and the 0 / 1023 corners
CLAMP_COLOURS_8 = [(235, 128, 240), (16, 16, 16), (16, 240, 240), (16, 128, 128), (235, 128, 128), (0, 0, 0), (255, 255, 255), (255, 0, 255), (0, 255, 0),
                   (255, 255, 0), (0, 0, 255), (128, 16, 240), (128, 240, 16)]
CORNERS = [(a, b, c) for a in (0, CMAX) for b in (0, CMAX) for c in (0, CMAX)]
PALETTE = [tuple(4 * x for x in col) for col in CLAMP_COLOURS_8] + [(g, 512, 512) for g in range(1024)] + CORNERS


def images(h, w, seed=0):
    """The three packed test frames of a size, uint8 [3, 6 * h * w] in the planar layout: random 10-bit samples; a binary 0 / 1023 one; one
    whose pixels are colours of PALETTE.  `relayout` turns one into x2rgb10le."""
    rng = np.random.default_rng(1000 * h + w + seed)
    rand = rng.integers(0, 1024, (3, h, w), dtype=np.int64)
    binary = rng.integers(0, 2, (3, h, w), dtype=np.int64) * CMAX
    pal = np.array(PALETTE, dtype=np.int64)
    y, x = np.mgrid[0:h, 0:w]
    idx = (y * 37 + x) % len(pal)                                           # 270 x 480 holds every colour
    return np.stack([pack_samples(rand, "yuv444p10le"), pack_samples(binary, "yuv444p10le"),
                     pack_samples(np.moveaxis(pal[idx], -1, 0), "yuv444p10le")])
