"""Integer numpy model of Pillow's 8-bit two-pass BILINEAR resize, driven by the tables the product hands to the library
(pythoncrt_amd.tables.pil_resample_axis): horizontal pass, its result rounded to uint8, then the vertical pass over that uint8 image.
tests/test_ingest_tables.py holds it to the installed Pillow byte for byte; the GPU tests then compare the kernels with Pillow itself."""
import numpy as np

from pythoncrt_amd import tables

# (src_h, src_w) -> (h, w): up, down, ragged, one axis unchanged, degenerate
PAIRS = [((48, 64), (96, 128)), ((45, 80), (67, 123)), ((108, 192), (54, 96)), ((97, 131), (33, 41)), ((30, 40), (90, 40)),
         ((30, 40), (30, 100)), ((1, 1), (5, 7)), ((7, 5), (1, 1)), ((120, 213), (119, 214)), ((16, 16), (40, 37)),
         ((270, 480), (540, 960)), ((3, 300), (200, 2))]
# the extra pairs of tests/test_ingest_gpu.py: a 1/40 down-scale (the general path by default) and row starts on every byte offset mod 4
EXTRA_PAIRS = [((360, 640), (9, 16))] + [((37, sw), (53, dw)) for sw, dw in zip((61, 62, 63, 64), (85, 86, 87, 88))]


def images(src_h, src_w, seed=0):
    """The two test images of a source size: seeded random bytes, and a random image of 0 / 255 only (every step is full scale)."""
    rng = np.random.default_rng([seed, src_h, src_w])
    return {"random": rng.integers(0, 256, (src_h, src_w, 3), dtype=np.uint8),
            "binary": (rng.integers(0, 2, (src_h, src_w, 3), dtype=np.uint8) * np.uint8(255))}


def resample_pass(img, xmin, count, k):
    """One pass along axis 1 of img (rows x n_in x channels, uint8) -> rows x n_out x channels uint8."""
    n_out, ksize = k.shape
    t = np.arange(ksize)[None, :]
    idx = np.minimum(xmin[:, None] + t, img.shape[1] - 1)                       # taps behind `count` carry k == 0
    kk = np.where(t < count[:, None], k, 0).astype(np.int64)
    acc = (1 << 21) + np.einsum("rxtc,xt->rxc", img[:, idx, :].astype(np.int64), kk)
    assert acc.min() >= 0 and acc.max() < 2 ** 31                               # the int32 accumulator of the C code never wraps
    return np.clip(acc >> 22, 0, 255).astype(np.uint8)


def resize(img, h, w):
    """Image.fromarray(img).resize((w, h), Image.BILINEAR) as integer arithmetic."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    hor = resample_pass(img, *tables.pil_resample_axis(img.shape[1], w))
    ver = resample_pass(np.ascontiguousarray(hor.transpose(1, 0, 2)), *tables.pil_resample_axis(img.shape[0], h))
    return np.ascontiguousarray(ver.transpose(1, 0, 2))


def pillow(img, h, w):
    from PIL import Image
    return np.asarray(Image.fromarray(np.ascontiguousarray(img, dtype=np.uint8)).resize((w, h), Image.BILINEAR))
