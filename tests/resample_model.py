"""Integer numpy model of the filtered resampler (include/crtfx_resample.h): Pillow's 8-bit two-pass resize with SIGNED taps — box, bilinear,
hamming, bicubic, lanczos — driven by the tables the product hands to the library (pythoncrt_amd.tables.pil_filter_axis).  The pass is an
int64 sum with an arithmetic shift and a clamp on both sides; `top` is 255 for uint8 images and 1020 for the quarter codes of half frames
(tests/resize16_model.py's quantiser and `to_half` around it).  tests/test_resample_tables.py holds the 8-bit model to the installed Pillow
byte for byte under all five filters; the GPU tests compare the uint8 kernels with Pillow itself and the half kernels with this model."""
import numpy as np

from pythoncrt_amd import tables
from tests import resize16_model

PREC = 22
QMAX = resize16_model.QMAX
FILTERS = tables.RESAMPLE_FILTERS
# the axes whose table facts were checked when the stage was specified, as (n_in, n_out)
SPEC_AXES = [(3840, 1920), (1920, 3840), (7680, 3840), (2160, 1080), (1080, 2160), (3840, 960), (640, 16), (131, 41), (213, 214), (4096, 1000),
             (1000, 4096)]


def masked(count, k):
    """The coefficients with the taps behind `count` zeroed: int64 [n_out, ksize]."""
    return np.where(np.arange(k.shape[1])[None, :] < count[:, None], k, 0).astype(np.int64)


def pass_sums(img, xmin, count, k):
    """The sums of one pass along axis 1 of img (rows x n_in x channels, integers) BEFORE the shift and the clamp: int64 rows x n_out x
    channels, 2^21 + sum k * in.  Blocks of 64 outputs are dense products of the block's source window with its weights, carried in
    float64 where every product and partial sum is an integer below 2^53 (asserted), so the result is the int64 sum exactly whatever the
    order of summation (tests/test_resample_tables.py holds it to a plain int64 sum): a 4K frame takes a second, not ten."""
    img = np.asarray(img)
    kk = masked(count, k)
    assert int(np.abs(kk).sum(axis=1).max()) * max(1, int(np.abs(img).max())) < 2 ** 52
    rows, n_in, ch = img.shape
    src = np.ascontiguousarray(img.transpose(0, 2, 1), dtype=np.float64).reshape(rows * ch, n_in)      # a row per (row, channel): a block is one GEMM
    n_out, ksize = k.shape
    t = np.arange(ksize)[None, :]
    acc = np.empty((rows * ch, n_out), dtype=np.int64)
    for o in range(0, n_out, 64):
        e = min(o + 64, n_out)
        s0, s1 = int(xmin[o:e].min()), int((xmin[o:e] + count[o:e]).max())
        live = t < count[o:e, None]
        W = np.zeros((s1 - s0, e - o), dtype=np.float64)
        W[(xmin[o:e, None] - s0 + t)[live], np.broadcast_to(np.arange(e - o)[:, None], live.shape)[live]] = kk[o:e][live]
        acc[:, o:e] = src[:, s0:s1] @ W                                           # exact integers: the cast loses nothing
    return np.ascontiguousarray(acc.reshape(rows, ch, n_out).transpose(0, 2, 1)) + (1 << (PREC - 1))


def resample_pass(img, xmin, count, k, top=255):
    """One pass along axis 1 of img (integers in 0..top) -> int64 in 0..top: clamp((2^21 + sum) >> 22, 0, top), the shift arithmetic."""
    img = np.asarray(img)
    assert img.min() >= 0 and img.max() <= top
    return np.clip(pass_sums(img, xmin, count, k) >> PREC, 0, top)


def resize_codes(q, h, w, filter, top=QMAX):
    """Integers 0..top [src_h, src_w, 3] -> [h, w, 3]: horizontal pass, rounded and clamped, then the vertical pass over its result."""
    hor = resample_pass(q, *tables.pil_filter_axis(q.shape[1], w, filter), top=top)
    ver = resample_pass(np.ascontiguousarray(hor.transpose(1, 0, 2)), *tables.pil_filter_axis(q.shape[0], h, filter), top=top)
    return np.ascontiguousarray(ver.transpose(1, 0, 2))


def resize_u8(img, h, w, filter):
    """Image.fromarray(img).resize((w, h), filter) as integer arithmetic: uint8 [src_h, src_w, 3] -> uint8 [h, w, 3]."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    return resize_codes(img, h, w, filter, top=255).astype(np.uint8)


def resize_half(frames, h, w, filter):
    """float16 [src_h, src_w, 3] or [n, src_h, src_w, 3] -> float16 [h, w, 3] / [n, h, w, 3]: quantise, both passes on quarter codes, half(q / 4)."""
    f = np.asarray(frames)
    assert f.dtype == np.float16
    if f.ndim == 4:
        return np.stack([resize_half(x, h, w, filter) for x in f])
    return resize16_model.to_half(resize_codes(resize16_model.quantise(f), h, w, filter, top=QMAX))


def resize_float(q, h, w, filter, top=QMAX):
    """The float64 restatement: the separable weighted sum with the float weights k / 2^22, no rounding between or behind the passes; it
    clamps to 0..top where the model does (behind either pass).  float64 [h, w, 3]."""
    def one(img, xmin, count, k):
        n_out, ksize = k.shape
        t = np.arange(ksize)[None, :]
        idx = np.minimum(xmin[:, None] + t, img.shape[1] - 1)
        kk = masked(count, k).astype(np.float64) / float(1 << PREC)
        return np.clip(np.einsum("rxtc,xt->rxc", img[:, idx, :], kk), 0.0, float(top))
    hor = one(np.asarray(q, dtype=np.float64), *tables.pil_filter_axis(q.shape[1], w, filter))
    ver = one(np.ascontiguousarray(hor.transpose(1, 0, 2)), *tables.pil_filter_axis(q.shape[0], h, filter))
    return np.ascontiguousarray(ver.transpose(1, 0, 2))


def pillow(img, h, w, filter):
    from PIL import Image
    return np.asarray(Image.fromarray(np.ascontiguousarray(img, dtype=np.uint8)).resize((w, h), getattr(Image, filter.upper())))


def fused_shape(src, dst, filter, bps):
    """(rows, cols, lds bytes) of the tile shape crtfx_resample_create takes for a pair, or None where no shape fits 40 960 bytes: the
    footprint formula of include/crtfx_resample.h with bps = 1 (uint8) or 2 (half) bytes a sample."""
    ax, ay = tables.pil_filter_axis(src[1], dst[1], filter), tables.pil_filter_axis(src[0], dst[0], filter)

    def extent(mn, cnt, n_out, tile):
        return max(int(mn[min(o + tile, n_out) - 1] + cnt[min(o + tile, n_out) - 1] - mn[o]) for o in range(0, n_out, tile))
    for TH, TW in ((32, 128), (32, 64), (16, 128), (16, 64), (8, 64), (8, 32), (4, 32)):
        rows, cols = min(TH, dst[0]), min(TW, dst[1])
        nr, nc = extent(ay[0], ay[1], dst[0], TH), extent(ax[0], ax[1], dst[1], TW)
        P, HP = (3 * bps * nc + 3 + 3) & ~3, ((3 * bps * cols + 3) & ~3) + 4
        total = 4 * (2 * cols + cols * ax[2].shape[1] + 2 * rows + rows * ay[2].shape[1]) + nr * (P + HP)
        if total <= 40960:
            return rows, cols, total
    return None
