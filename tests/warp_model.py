"""The float32-storage model of the warp / commit stage (a12 - a15): what k_warp, k_warp_lean and its commit-only form must produce, bit for bit.

The oracle interpolates the reference's float64 image; the GPU interpolates the pre-warp image it stored as float32, and keeps the
persistence state as float32 between frames.  Those two roundings are the whole difference, so the model is the oracle's
own functions composed with them and contains no arithmetic of its own:

  * pre-warp image: the oracle's chain with the warp off, `.astype(float32)` (the suite holds that to the GPU bit for bit); float32 for an
    unpromoted chain (no vignette, no flicker), widened again to float64 for a promoted one — the dtype the reference's image has there;
  * warped image: orc.remap_bilinear(pre, *orc.barrel_maps(h, w, s)) in that dtype; the static float result is its `.astype(float32)`.
    In float64 every product of a float32-valued tap and a float32 weight is exact, so OpenCV's two summation forms (VARIANT["remap_fma"]:
    multiply-then-add, or contracted) round the same real numbers and the model is the same under both; in float32 the oracle's and the
    kernels' form is multiply-then-add, left to right;
  * glitch band: orc._apply_glitch, a pure gather (it commutes with the narrowing);
  * render commit: orc.persistence_blend's expression on the previous state held as float32 (widened to the image's dtype), the first frame
    passing through unblended; the state is `.astype(float32)` after every frame, the uint8 frame orc.convert_scale_abs of that float32
    state, the half frame np.abs(state32 * float32(255)).astype(float16);
  * preview commit: orc.add_weighted on the float32-held state, the same narrowing.

point_render is the same composition for the pointwise chain (no warp, fast or no bloom: tests/point_builds.py), where no pre-warp image is
parked: the image reaches the blend un-narrowed, in the reference's own dtype, and only the state is float32.

Only numpy and the oracle: nothing here imports torch or the package."""
import contextlib

import numpy as np

from oracle import crt_oracle as orc

PARAM_KEYS = ("scanline_strength", "triad_gamma", "triad_preserve_luma", "aberration_px", "bloom_sigma", "bloom_strength", "bloom_threshold",
              "noise_strength", "scanline_period_px", "fast_bloom", "pixel_size", "warp_strength")

# every gate off: the pre-warp image is exactly float32(u8) / 255 (half frames: float32(half) / 255) and the chain stays float32
OFF = dict(scanline_strength=0.0, triad_strength=0.0, triad_softness=0.0, triad_gamma=2.2, triad_preserve_luma=False, aberration_px=0,
           bloom_sigma=0.0, bloom_strength=0.0, bloom_threshold=0.0, noise_strength=0.0, vignette_strength=0.0, scanline_period_px=2.0,
           scanline_speed_px_s=30.0, fast_bloom=False, pixel_size=1, warp_strength=0.0, persistence=0.0)
# the full-chain gate set (BASELINE configs 2 - 5): Gaussian bloom, softened triad, scanlines, vignette (promotes to float64), grain
FULL = dict(OFF, scanline_strength=0.6, triad_strength=0.35, triad_softness=0.5, aberration_px=1, bloom_sigma=1.2, bloom_strength=0.25,
            noise_strength=1.5, vignette_strength=0.25)
# a promoted chain without a grain plane (scanlines + vignette): the render loop groups its frames into multi-frame launches
VIG = dict(OFF, scanline_strength=0.6, vignette_strength=0.25)
# Gaussian bloom alone (float32) / with the vignette (float64): with the warp off a persistence chain behind it takes the commit-only build
BLOOM32 = dict(OFF, bloom_sigma=1.2, bloom_strength=0.25)
BLOOM64 = dict(BLOOM32, vignette_strength=0.25)


def promoted(cfg):
    """The reference's image is float64 behind the vignette (its mask is float64) or the flicker (a Python float times ... np.sin)."""
    return cfg.get("vignette_strength", 0.0) > 0.0 or (cfg.get("flicker_strength", 0.0) > 0.0 and cfg.get("flicker_hz", 0.0) > 0.0)


# the keywords of the pointwise chain's settings (tests/point_builds.py): the colour grade, flicker, coarse grain, the 2-D scanline plane
POINT_KEYS = ("brightness", "contrast", "gamma", "saturation", "temperature", "flicker_strength", "flicker_hz", "grain_size", "scanline_angle",
              "scanline_thickness")


def _params(cfg, **over):
    p = {k: cfg[k] for k in PARAM_KEYS}
    p.update({k: cfg[k] for k in POINT_KEYS + ("glitch_amp_px", "glitch_height_frac") if k in cfg})
    p.update(over)
    return p


@contextlib.contextmanager
def injected_scan_plane(plane):
    """The oracle's chain with its 2-D scanline mask (make_scanline_mask_2d: float64 sin / pow, returned float32) replaced by `plane`, the
    float32 mask the GPU generated (crtfx_scanline_plane, held to the oracle's within one ulp by tests/test_parity_gpu.py) — an input handed
    in, as the grain planes are; None: the oracle's own mask."""
    if plane is None:
        yield
        return
    own = orc.make_scanline_mask_2d
    orc.make_scanline_mask_2d = lambda h, w, *a: np.ascontiguousarray(plane, np.float32).reshape(h, w)
    try:
        yield
    finally:
        orc.make_scanline_mask_2d = own


def oracle_render(frames, cfg, fps=30.0, first=0, planes=None, state=None):
    """The unmodified oracle's in-order render, one frame at a time: -> (uint8 frames, per-frame states in the oracle's own dtype)."""
    outs, states = [], []
    for j, f in enumerate(frames):
        o, state = orc.process_frames([f], _params(cfg), fps, cfg["scanline_speed_px_s"], cfg["persistence"], cfg["triad_strength"],
                                      cfg["triad_softness"], cfg["vignette_strength"], noise_planes=None if planes is None else [planes[j]],
                                      first_index=first + j, prev_state=state)
        outs.append(o[0])
        states.append(state)
    return outs, states


def pre_images(frames, cfg, fps=30.0, first=0, planes=None, scan_planes=None, parked=True):
    """The pre-warp image of every frame as the GPU holds it: the oracle's chain with warp, glitch and persistence off, narrowed to float32;
    widened back to float64 when the chain is promoted.  scan_planes: per-frame 2-D scanline masks to hand in (injected_scan_plane).
    parked=False: the image in the oracle's own dtype, never narrowed (the pointwise chain: see point_render)."""
    off = dict(cfg, warp_strength=0.0, persistence=0.0, glitch_amp_px=0, glitch_height_frac=0.0)
    out = []
    for j, f in enumerate(frames):
        with injected_scan_plane(None if scan_planes is None else scan_planes[j]):
            _, st = orc.process_frames([f], _params(off), fps, off["scanline_speed_px_s"], 0.0, off["triad_strength"], off["triad_softness"],
                                       off["vignette_strength"], noise_planes=None if planes is None else [planes[j]], first_index=first + j)
        assert st.dtype == (np.float64 if promoted(cfg) else np.float32), (st.dtype, promoted(cfg))
        out.append(st.astype(np.float32).astype(st.dtype) if parked else st)
    return out


def warp(pre, strength, glitch=None):
    """The warped (and glitched) image in the chain's dtype.  glitch: None or (y0, int32 offsets) as orc.glitch_offsets_* return them."""
    img = pre
    if float(strength) != 0.0:
        h, w = pre.shape[:2]
        img = orc.remap_bilinear(pre, *orc.barrel_maps(h, w, float(strength)))
    if glitch is not None and glitch[1] is not None:
        img = orc._apply_glitch(np.array(img), glitch[0], glitch[1])
    return img


def static_image(pre, strength, glitch=None):
    """apply_static_effects' float image as the GPU returns it (float32)."""
    return warp(pre, strength, glitch).astype(np.float32)


def to_u8(state32):
    assert state32.dtype == np.float32
    return orc.convert_scale_abs(state32, 255.0)


def to_half(state32):
    assert state32.dtype == np.float32
    return np.abs(state32 * np.float32(255.0)).astype(np.float16)


def quantise(state32, half):
    return to_half(state32) if half else to_u8(state32)


def render_chain(images, persistence, state=None):
    """The render loop's in-order commit (ref:1086-1098) of warped images: -> per-frame float32 states.  `state`: the float32 state carried
    in, or None at the start of a clip (the first frame then passes through unblended)."""
    states = []
    for img in images:
        prev = None if state is None else np.asarray(state, np.float32).astype(img.dtype)
        blended, _ = orc.persistence_blend(prev, img, persistence)
        state = blended.astype(np.float32)
        states.append(state)
    return states


def render(frames, cfg, half=False, fps=30.0, first=0, planes=None, state=None, scan_planes=None, parked=True):
    """FramePipeline.run under the model: -> (frames as uint8 / half, per-frame float32 states)."""
    imgs = [warp(p, cfg["warp_strength"]) for p in pre_images(frames, cfg, fps, first, planes, scan_planes, parked)]
    if cfg["persistence"] > 0.0:
        states = render_chain(imgs, cfg["persistence"], state)
    else:
        states = [i.astype(np.float32) for i in imgs]
    return [quantise(s, half) for s in states], states


def point_render(frames, cfg, half=False, fps=30.0, first=0, planes=None, state=None, scan_planes=None):
    """A render run of the pointwise chain (fast or no bloom, warp off) under the model.  Nothing parks a pre-warp image there: the pointwise
    kernels blend the image in the dtype the reference has it in (float64 once the vignette or the flicker promotes), in registers —
    st = (float)clip01(p * (T)st + q * v) — so the float32 storage of the STATE is the model's one rounding and the image is the oracle's
    own, un-narrowed (render's default narrows it first: the float32 image k_warp_lean and the commit-only build read back)."""
    assert float(cfg["warp_strength"]) == 0.0
    return render(frames, cfg, half, fps, first, planes, state, scan_planes, parked=False)


def preview_step(img, persistence, state=None):
    """apply_crt_effect's commit (ref:687-699) of one warped image: -> (uint8 frame, float32 state)."""
    if state is not None and persistence > 0.0:
        img = orc.add_weighted(np.asarray(state, np.float32).astype(img.dtype), float(persistence), img, float(1.0 - persistence))
    s32 = img.astype(np.float32)
    return to_u8(s32), s32


# ---- the pixel classes of a geometry -----------------------------------------------------------------------------------------------
CLASSES = ("all-in", "x-partial", "y-partial", "xy-partial", "all-out", "iy-clamped", "ix-clamped")


def census(h, w, strength):
    """Counts of CLASSES over the h x w output pixels of the barrel map: how many of the four taps lie inside the image (the first five
    classes partition the pixels), and the two ranges k_warp_lean clamps before its 24-bit multiply (iy < -2 or iy > H, ix < -1 or ix > W)."""
    ix, iy, _ = orc.remap_quantise(*orc.barrel_maps(h, w, float(strength)))
    nx = ((ix >= 0) & (ix < w)).astype(int) + ((ix + 1 >= 0) & (ix + 1 < w))
    ny = ((iy >= 0) & (iy < h)).astype(int) + ((iy + 1 >= 0) & (iy + 1 < h))
    return {"all-in": int(((nx == 2) & (ny == 2)).sum()), "x-partial": int(((nx == 1) & (ny == 2)).sum()),
            "y-partial": int(((nx == 2) & (ny == 1)).sum()), "xy-partial": int(((nx == 1) & (ny == 1)).sum()),
            "all-out": int(((nx == 0) | (ny == 0)).sum()), "iy-clamped": int(((iy < -2) | (iy > h)).sum()),
            "ix-clamped": int(((ix < -1) | (ix > w)).sum())}


def zero_fraction_share(h, w, strength):
    """Share of the pixels whose x or y fraction is exactly 0 (the right / bottom tap then has weight 0)."""
    _, _, fxy = orc.remap_quantise(*orc.barrel_maps(h, w, float(strength)))
    return float((((fxy & 31) == 0) | ((fxy >> 5) == 0)).mean())


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
STRENGTHS = (0.15, 1.0, 2.5, -0.4, -1.0, 1e-3, -1e-3)
SHAPES = ((1, 1), (3, 5), (2, 64), (17, 63), (33, 65), (16, 128), (37, 129), (40, 132), (31, 190), (70, 130), (24, 256), (135, 240), (9, 1028))


def make_frame(h, w, seed, half=False):
    """A frame with structure in both axes and noise on top; half: fractional values on the 0..255 scale."""
    rng = np.random.default_rng(seed)
    if half:
        return (rng.random((h, w, 3), dtype=np.float32) * 255.0).astype(np.float16)
    yy, xx = np.mgrid[0:h, 0:w]
    g = np.stack([(xx * 255) // max(1, w - 1), (yy * 255) // max(1, h - 1), ((xx + yy) * 255) // max(1, h + w - 2)], axis=2)
    return np.clip((g + rng.integers(0, 64, (h, w, 3))) // 2 + 40 + rng.integers(-40, 40, (h, w, 3)), 0, 255).astype(np.uint8)


def make_plane(h, w, seed):
    return np.random.default_rng(seed).standard_normal((h, w), dtype=np.float32)


def make_state(h, w, seed):
    """A float32 persistence state in [0, 1] with full 24-bit mantissas."""
    return np.random.default_rng(seed).random((h, w, 3), dtype=np.float32)
