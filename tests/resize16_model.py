"""Integer numpy model of the half resampler (include/crtfx_resize16.h): Pillow's 8-bit two-pass BILINEAR resize on the quarter-code scale
of the 10-bit stages, driven by the tables the product hands to the library (pythoncrt_amd.tables.pil_resample_axis).  Half frames are
quantised to quarter codes 0..1020, resampled horizontally, the result a quarter code, resampled vertically, and written as half(q / 4).
`resample_pass` with top=255 on uint8 images IS tests/pil_resize_model.resample_pass (tests/test_resize16_tables.py holds the two to each
other, and through that one to the installed Pillow byte for byte); with top=1020 it is the pass of the kernels."""
import numpy as np

from pythoncrt_amd import tables

QMAX = 1020
PREC = 22
# the full-size pairs whose accumulator bound was checked when the stage was specified, as (n_in, n_out) axes
FULL_AXES = [(3840, 1920), (2160, 1080), (1920, 3840), (1080, 2160), (7680, 1920), (4320, 1080), (7680, 3840), (4320, 2160), (4096, 1000), (131, 40),
             (32767, 1), (32767, 16), (1, 32767), (1920, 1280), (1280, 1920), (720, 1080), (1080, 720)]


def quantise(half):
    """q = rint_to_even(min(max(4 f, 0), 1020)), NaN -> 0, of float16 values: int64.  4 f is exact in float64 as it is in float32."""
    half = np.asarray(half)
    assert half.dtype == np.float16
    with np.errstate(invalid="ignore"):             # signalling NaN patterns
        t = 4.0 * half.astype(np.float64)
        t = np.where(t > 0.0, t, 0.0)               # NaN, -0, negatives, -inf -> 0
    return np.rint(np.minimum(t, float(QMAX))).astype(np.int64)


def to_half(q):
    """half(q / 4): exact for every quarter code."""
    return (np.asarray(q, dtype=np.float64) / 4.0).astype(np.float16)


def resample_pass(img, xmin, count, k, top=QMAX):
    """One pass along axis 1 of img (rows x n_in x channels, integers in 0..top) -> rows x n_out x channels int64 in 0..top."""
    img = np.asarray(img)
    assert img.min() >= 0 and img.max() <= top
    img = img.astype(np.uint16)                                                 # top <= 1020: the gathers below move a quarter of the bytes
    n_out, ksize = k.shape
    t = np.arange(ksize)[None, :]
    idx = np.minimum(xmin[:, None] + t, img.shape[1] - 1)                       # taps behind `count` carry k == 0
    kk = np.where(t < count[:, None], k, 0).astype(np.int64)
    assert (1 << (PREC - 1)) + top * int(kk.sum(axis=1).max()) < 2 ** 32        # what crtfx_resize16_create admits (top = 1020)
    acc = np.full((img.shape[0], n_out, img.shape[2]), 1 << (PREC - 1), dtype=np.int64)
    for j in range(ksize):                                                      # tap by tap: a 4K frame stays a few hundred megabytes
        if kk[:, j].any():
            acc += img[:, idx[:, j], :] * kk[:, j][None, :, None]
    assert acc.min() >= 0 and acc.max() < 2 ** 32                               # the uint32 accumulator never wraps
    return np.minimum(acc >> PREC, top)


def resize_codes(q, h, w):
    """Quarter codes int64 [src_h, src_w, 3] -> [h, w, 3]: horizontal pass, then the vertical pass over its quarter codes."""
    hor = resample_pass(q, *tables.pil_resample_axis(q.shape[1], w))
    ver = resample_pass(np.ascontiguousarray(hor.transpose(1, 0, 2)), *tables.pil_resample_axis(q.shape[0], h))
    return np.ascontiguousarray(ver.transpose(1, 0, 2))


def resize(frames_f16, h, w):
    """float16 [src_h, src_w, 3] or [n, src_h, src_w, 3] -> float16 [h, w, 3] / [n, h, w, 3]."""
    f = np.asarray(frames_f16)
    assert f.dtype == np.float16
    if f.ndim == 4:
        return np.stack([resize(x, h, w) for x in f])
    return to_half(resize_codes(quantise(f), h, w))


def resize_float(q, h, w):
    """The float64 restatement: the exact separable weighted mean of quarter codes with the float weights k / 2^22, no rounding between or
    behind the passes.  float64 [h, w, 3]."""
    def one(img, xmin, count, k):
        n_out, ksize = k.shape
        t = np.arange(ksize)[None, :]
        idx = np.minimum(xmin[:, None] + t, img.shape[1] - 1)
        kk = np.where(t < count[:, None], k, 0).astype(np.float64) / float(1 << PREC)
        return np.einsum("rxtc,xt->rxc", img[:, idx, :], kk)
    hor = one(np.asarray(q, dtype=np.float64), *tables.pil_resample_axis(q.shape[1], w))
    ver = one(np.ascontiguousarray(hor.transpose(1, 0, 2)), *tables.pil_resample_axis(q.shape[0], h))
    return np.ascontiguousarray(ver.transpose(1, 0, 2))


SPECIALS = np.array([0x7E00, 0xFE00, 0x7C01, 0x7C00, 0xFC00, 0x8000, 0x0000, 0x0001, 0x8001, 0x5BF8, 0x5BF9, 0x5C00, 0x7BFF, 0xFBFF, 0x3000, 0x2FFF, 0x3001],
                    dtype=np.uint16)      # NaNs, +-inf, +-0, denormals, 255.0 and its neighbours, +-max, 0.125 (a tie of 4 f) and its neighbours


def images(src_h, src_w, seed=0):
    """The two test images of a source size, float16 [src_h, src_w, 3]: "random" — seeded random halves over the whole range of the format
    (random bit patterns, so negatives, values above 255, NaN and +-inf occur; half of the elements are drawn inside 0..255 with every
    fraction; SPECIALS is scattered over it) — and "binary", 0 / 255.0 only (every step is full scale)."""
    rng = np.random.default_rng([seed, src_h, src_w, 16])
    n = src_h * src_w * 3
    bits = rng.integers(0, 1 << 16, n, dtype=np.int64).astype(np.uint16)
    inside = (rng.random(n) * 260.0 - 2.0).astype(np.float16).view(np.uint16)
    bits = np.where(rng.random(n) < 0.5, inside, bits)
    pos = rng.integers(0, n, max(1, n // 7))
    bits[pos] = SPECIALS[rng.integers(0, len(SPECIALS), pos.size)]
    binary = (rng.integers(0, 2, n, dtype=np.int64) * 255).astype(np.float16)
    return {"random": bits.view(np.float16).reshape(src_h, src_w, 3), "binary": binary.reshape(src_h, src_w, 3)}
