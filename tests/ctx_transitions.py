"""Parameter sets ("stops") a long-lived ctx is walked through, and the walks: the table that drives tests/test_ctx_transitions.py (CPU: every
step of every walk changes the picture enough that a stale table would show) and tests/test_ctx_transitions_gpu.py (a ctx reused across the
walk against a ctx created for each stop, bit for bit, same crtfx_last_plan).  No torch import here.

A stop is a set of RenderSettings overrides on BASE — the full chain: Gaussian bloom sigma 3, softened triad through its LUTs, row
scanlines, analytic vignette, grain, warp 0.15 — plus three keys that are not RenderSettings fields:

  _planes    the triad mask and the vignette handed in as plain per-pixel arrays (the LDS-ring kernel); `api` only: RenderSettings builds
             its masks from strengths
  _overlay   "before" | "after": a text overlay plane; `api` only: a FramePipeline keeps its overlay for its lifetime

Routes: `api` = apply_static_effects (the float image) + apply_crt_effect (frame and state) on the drop-in's cached Engine; `loop` =
FramePipeline.run after FramePipeline.set_settings.

`family` says which crtfx_last_plan entry the stop must land on: {"route/pix/size" pattern: "key=prefix"}, first matching pattern wins
(fnmatch; size is "even" or "odd").  Why the patterns differ by size and format (pythoncrt_amd/csrc/crtfx.hip, launch_rr_group):
  * the full-chain gate set with a pre-warp image parked (warp, or the loop's persistence) runs k_phosphor_ct up to radius 15, k_phosphor_cc
    above (uint8) / k_phosphor_rr (half);
  * k_phosphor_ct reads uint8 frames as dwords and half frames as qwords: the loop's later frames of the odd size (23 x 131: 9039 / 18078
    bytes per frame) do not start on such a boundary and take k_phosphor_cc (uint8) / k_phosphor_rr (half) — same bits;
  * any other gate set runs k_phosphor_rr (its run-time or +pixelate build); per-pixel planes the LDS-ring kernel k_phosphor<-1>;
  * radius >= 31 is the split bloom (k_sb_rows + k_sb_cols in front of the pointwise kernel);
  * fast bloom: k_half + k_point_sel for one frame; in the loop the fused kernel on the even size (exact 2x decimation), k_half_group +
    k_point_lean_seq on the odd one (the fbd_* tap tables).
k_point<runtime> is reached through CRTFX_OPT_FORCE_GENERIC only, which is handed to a ctx when it is created: not a stop of a walk.

Every stop reaches its family at the two sizes of SIZES; no size had to change."""
import fnmatch
import random
from dataclasses import dataclass

import numpy as np

SIZES = {"even": (24, 136), "odd": (23, 131)}          # 136 = 2 x 64 + 8: two whole strips and a partial one, a multiple of 8; 23 x 131: odd, ragged
PIXES = ("u8", "half")
ROUTES = ("api", "loop")

# the full chain (RenderSettings field names)
BASE = dict(scanline_strength=0.6, triad_strength=0.35, triad_gamma=2.2, triad_preserve_luma=False, triad_softness=0.5, aberration_px=1,
            bloom_sigma=3.0, bloom_strength=0.25, bloom_threshold=0.0, noise_strength=1.5, vignette_strength=0.25, persistence=0.5,
            scanline_speed_px_s=30.0, scanline_period_px=2.0, fast_bloom=False, pixel_size=1, brightness=0.0, contrast=1.0, gamma=1.0,
            saturation=1.0, temperature=0.0, flicker_strength=0.0, flicker_hz=0.0, grain_size=1, scanline_angle=0.0,
            scanline_thickness=1.0, warp_strength=0.15, glitch_amp_px=0, glitch_height_frac=0.0)

CT, CC, RR = "phosphor=k_phosphor_ct<", "phosphor=k_phosphor_cc<", "phosphor=k_phosphor_rr<"
FOLDED = {"api/*/*": CT, "loop/*/even": CT, "loop/u8/odd": CC, "loop/half/odd": RR}      # the full-chain gate set, radius <= 15
RUNTIME = {"*": RR}                                                                          # any other gate set in front of a Gaussian bloom
SPLIT = {"*": "blur=k_sb_rows<"}


@dataclass(frozen=True)
class Stop:
    name: str
    settings: dict
    family: dict
    routes: tuple = ROUTES
    pixes: tuple = PIXES
    note: str = ""

    def config(self):
        return dict(BASE, **{k: v for k, v in self.settings.items() if not k.startswith("_")})

    def family_for(self, route, pix, size):
        key = f"{route}/{pix}/{size}"
        for pat, fam in self.family.items():
            if fnmatch.fnmatchcase(key, pat if pat.count("/") == 2 else "*"):
                return fam.split("=", 1)
        raise KeyError((self.name, key))


S5 = dict(bloom_strength=0.5)          # the tap pairs are the tight ones: at bloom strength 0.5 every pair clears the 5 % / 1 % conditions

STOPS = (
    Stop("full", {}, FOLDED),
    # ---- fast bloom: ds holds the half-resolution slots; the odd size uses the fbd_* tap tables and k_half
    Stop("cli_defaults", dict(fast_bloom=True, pixel_size=2, warp_strength=0.0, bloom_sigma=1.2),
         {"api/*/*": "point=k_point_sel<", "loop/*/even": "point=k_point_fused_seq<", "loop/*/odd": "point=k_point_lean_seq<"}),
    Stop("fast_bloom", dict(fast_bloom=True), {"loop/*/even": "point=k_point_fused_seq<", "*/*/*": "half=k_half"}),
    # ---- pixelate: xmap / ymap, W and H int32 each, whatever the cell
    Stop("pix2", dict(pixel_size=2), RUNTIME),
    Stop("pix3", dict(pixel_size=3), RUNTIME),
    # ---- grade: the 3 x 256 table of uint8 frames keeps its size and changes its content, then is dropped (a saturation cannot be tabled)
    Stop("grade_a", dict(brightness=0.05, contrast=1.1, gamma=0.9), RUNTIME),
    Stop("grade_b", dict(gamma=1.3, temperature=-0.5), RUNTIME),
    Stop("grade_sat", dict(saturation=1.4), RUNTIME),
    # ---- Gaussian taps
    Stop("taps_0p9", dict(S5, bloom_sigma=0.9), FOLDED, note="radius 3"),
    Stop("taps_1p1", dict(S5, bloom_sigma=1.1), FOLDED, note="radius 3, other taps"),
    Stop("taps_2p9", dict(S5, bloom_sigma=2.9), FOLDED, note="radius 9"),
    Stop("taps_3p1", dict(S5, bloom_sigma=3.1), FOLDED, note="radius 9, other taps"),
    Stop("taps_5p5", dict(S5, bloom_sigma=5.5), {"*/u8/*": CC, "*/half/*": RR}, note="radius 16: past k_phosphor_ct"),
    Stop("taps_11p0", dict(S5, bloom_sigma=11.0), SPLIT, note="radius 33: split bloom, tpad"),
    Stop("taps_11p1", dict(S5, bloom_sigma=11.1), SPLIT, note="radius 33, other taps, the same tpad length"),
    Stop("taps_20", dict(S5, bloom_sigma=20.0), SPLIT, note="radius 60: the tpad buffer grows; 11.0 after it is a shorter array in the larger buffer"),
    # ---- triad: the mask row, lut_g / lut_inv, the composite tables of k_phosphor_ct
    Stop("triad_soft1p4", dict(triad_softness=1.4), FOLDED),
    Stop("triad_gamma1p8", dict(triad_gamma=1.8), FOLDED, note="both LUTs and the composite tables keep their size"),
    Stop("triad_luma", dict(triad_softness=1.4, triad_preserve_luma=True), RUNTIME, note="composite tables off"),
    Stop("triad_gamma1", dict(triad_softness=1.4, triad_gamma=1.0), RUNTIME, note="no LUT path"),
    Stop("triad_off", dict(triad_strength=0.0), RUNTIME),
    # ---- vignette
    Stop("vig_1p0", dict(vignette_strength=1.0), FOLDED),
    Stop("vig_off", dict(vignette_strength=0.0), RUNTIME),
    # ---- grain: the resize axes of coarse grain, W and H entries whatever the cell
    Stop("grain2", dict(grain_size=2), RUNTIME),
    Stop("grain3", dict(grain_size=3), RUNTIME),
    Stop("grain_off", dict(noise_strength=0.0), RUNTIME),
    # ---- warp: the same axis tables, other scalars; the warp kernels themselves
    Stop("warp_neg", dict(warp_strength=-0.3), {"api/*/*": "warp=k_warp<", "loop/*/*": "warp=k_warp_lean<"}),
    Stop("warp_off", dict(warp_strength=0.0), dict(FOLDED, **{"api/*/*": RR}), note="api: no image parked, the register-window kernel"),
    # ---- scanlines
    Stop("scan_2d", dict(scanline_angle=12.0, scanline_thickness=2.0), RUNTIME),
    Stop("scan_off", dict(scanline_strength=0.0), RUNTIME),
    # ---- aberration
    Stop("ab_m3", dict(aberration_px=-3), FOLDED),
    Stop("ab_0", dict(aberration_px=0), FOLDED),
    # ---- bloom threshold
    Stop("thr_0p2", dict(bloom_threshold=0.2), RUNTIME),
    Stop("thr_0p4", dict(bloom_threshold=0.4), RUNTIME),
    # ---- per-pixel planes
    Stop("planes", dict(_planes=True), {"*": "phosphor=k_phosphor<-1>"}, routes=("api",)),
    # ---- text overlay
    Stop("overlay_before", dict(_overlay="before"), RUNTIME, routes=("api",)),
    Stop("overlay_after", dict(_overlay="after"), {"*": "warp=k_warp<"}, routes=("api",)),
    # ---- glitch (api: render variant for the float image, preview variant for the frame)
    Stop("glitch_on", dict(glitch_amp_px=7, glitch_height_frac=0.3), {"api/*/*": "warp=k_warp<", "loop/*/even": CT, "loop/u8/odd": CC, "loop/half/odd": RR}),
)
BY_NAME = {s.name: s for s in STOPS}
assert len(BY_NAME) == len(STOPS)


@dataclass(frozen=True)
class Arrow:
    a: str
    b: str
    same: tuple = ()        # host tables both stops upload with the same byte size and different content
    drops: tuple = ()       # host tables `a` uploads and `b` does not (the other direction: goes on after it was off)
    pix: tuple = PIXES      # formats the table statement holds for (the grade table exists for uint8 frames only)


# consecutive stops of the groups; tests walk every arrow in both directions
ARROWS = (
    Arrow("full", "cli_defaults", drops=("taps",)), Arrow("cli_defaults", "fast_bloom"),
    Arrow("pix2", "pix3", same=("pixelate",)), Arrow("pix3", "full", drops=("pixelate",)),
    Arrow("grade_a", "grade_b", same=("grade_lut",), pix=("u8",)), Arrow("grade_b", "grade_sat", drops=("grade_lut",), pix=("u8",)), Arrow("grade_sat", "full"),
    Arrow("taps_0p9", "taps_1p1", same=("taps",)), Arrow("taps_2p9", "taps_3p1", same=("taps",)), Arrow("taps_3p1", "taps_5p5"),
    Arrow("taps_11p0", "taps_11p1", same=("taps",)), Arrow("taps_20", "taps_11p0"),
    Arrow("full", "fast_bloom", drops=("taps",)), Arrow("fast_bloom", "taps_11p0"),
    Arrow("full", "triad_soft1p4", same=("triad_row",)), Arrow("full", "triad_gamma1p8", same=("triad_luts",)),
    Arrow("triad_soft1p4", "triad_luma"), Arrow("triad_luma", "triad_gamma1", drops=("triad_luts",)), Arrow("triad_gamma1", "triad_off", drops=("triad_row",)),
    Arrow("full", "vig_1p0"), Arrow("vig_1p0", "vig_off"),
    Arrow("grain2", "grain3", same=("grain_axes",)), Arrow("grain3", "full", drops=("grain_axes",)), Arrow("full", "grain_off"),
    Arrow("full", "warp_neg", same=("warp_scalars",)), Arrow("warp_neg", "warp_off", drops=("warp_scalars",)),
    Arrow("scan_2d", "full"), Arrow("full", "scan_off"),
    Arrow("full", "ab_m3"), Arrow("ab_m3", "ab_0"),
    Arrow("thr_0p2", "thr_0p4"), Arrow("thr_0p4", "full"),
    Arrow("planes", "full"),
    Arrow("overlay_before", "overlay_after"), Arrow("overlay_after", "full"),
    Arrow("glitch_on", "full"),
)

RANDOM_SEED, RANDOM_STEPS = 20260, 40


def stops_of(route, pix):
    return [s.name for s in STOPS if route in s.routes and pix in s.pixes]


def _chain(parts):
    out = []
    for p in parts:
        for name in p:
            if not out or out[-1] != name:
                out.append(name)
    return out


def star_walk(route, pix):
    """base -> X -> base for every stop X of the route."""
    return _chain([("full", x, "full") for x in stops_of(route, pix) if x != "full"])


def pairs_walk(route, pix):
    """Every arrow in both directions: a -> b -> a."""
    ok = set(stops_of(route, pix))
    return _chain([(ar.a, ar.b, ar.a) for ar in ARROWS if ar.a in ok and ar.b in ok])


def random_walk(route, pix):
    """One seeded walk of RANDOM_STEPS steps over all stops of the route (no stop twice in a row)."""
    names = stops_of(route, pix)
    rng = random.Random(RANDOM_SEED)
    out = ["full"]
    while len(out) <= RANDOM_STEPS:
        nxt = rng.choice(names)
        if nxt != out[-1]:
            out.append(nxt)
    return out


WALKS = {"star": star_walk, "pairs": pairs_walk, "random": random_walk}


def steps(walk):
    return list(zip(walk[:-1], walk[1:]))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def make_frame(h, w, seed, half=False):
    """A gradient in both axes plus noise (half: fractional values on the 0..255 scale)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    g = np.stack([(xx * 255.0) / max(1, w - 1), (yy * 255.0) / max(1, h - 1), ((xx + yy) * 255.0) / max(1, h + w - 2)], axis=2)
    f = np.clip(0.5 * g + 0.5 * rng.random((h, w, 3)) * 255.0, 0.0, 255.0)
    return f.astype(np.float16) if half else f.astype(np.uint8)


def make_state(h, w, seed):
    return np.random.default_rng(seed).random((h, w, 3), dtype=np.float32)


def make_overlay(h, w, seed):
    """An RGBA plane: the upper quarter untouched, a translucent block, an opaque lower part."""
    rng = np.random.default_rng(seed)
    ov = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    ov[: h // 4, :, 3] = 0
    ov[h // 2:, :, 3] = 255
    return ov


def plane_masks(h, w, seed):
    """(H x W x 3 float32 triad plane, H x W float64 vignette plane) with no structure a descriptor could encode."""
    rng = np.random.default_rng(seed)
    return (0.5 + 0.5 * rng.random((h, w, 3))).astype(np.float32), 0.5 + 0.5 * rng.random((h, w))


API_KEYS = ("brightness", "contrast", "gamma", "saturation", "temperature", "flicker_strength", "flicker_hz", "grain_size", "scanline_angle",
            "scanline_thickness", "warp_strength")
PHASE, TIME_SEC = 1.25, 0.12


def api_masks(mod, stop, h, w):
    """(triad mask, vignette mask) of a stop as module `mod` (the drop-in or the oracle) builds them; planes are plain arrays for both."""
    cfg = stop.config()
    if stop.settings.get("_planes"):
        return plane_masks(h, w, 5)
    tm = mod.make_triad_mask(h, w, cfg["triad_strength"], cfg["triad_softness"]) if cfg["triad_strength"] > 0.0 else None
    vg = mod.make_vignette(h, w, cfg["vignette_strength"]) if cfg["vignette_strength"] > 0.0 else None
    return tm, vg


def api_keywords(stop, h, w):
    cfg = stop.config()
    kw = {k: cfg[k] for k in API_KEYS}
    if stop.settings.get("_overlay"):
        kw["text_overlay_rgba"], kw["text_overlay_after"] = make_overlay(h, w, 9), stop.settings["_overlay"] == "after"
    return kw


def static_args(frame, masks, cfg):
    """apply_static_effects' positional arguments."""
    return (frame, cfg["scanline_strength"], masks[0], cfg["triad_gamma"], cfg["triad_preserve_luma"], cfg["aberration_px"], cfg["bloom_sigma"],
            cfg["bloom_strength"], cfg["bloom_threshold"], cfg["noise_strength"], masks[1], cfg["scanline_period_px"], PHASE, cfg["fast_bloom"],
            cfg["pixel_size"], cfg["glitch_amp_px"], cfg["glitch_height_frac"])


def crt_args(frame, masks, cfg, persistence, state):
    """apply_crt_effect's positional arguments."""
    return (frame, cfg["scanline_strength"], masks[0], cfg["triad_gamma"], cfg["triad_preserve_luma"], cfg["aberration_px"], cfg["bloom_sigma"],
            cfg["bloom_strength"], cfg["bloom_threshold"], cfg["noise_strength"], masks[1], persistence, state, cfg["scanline_period_px"], PHASE,
            cfg["fast_bloom"], cfg["pixel_size"], cfg["glitch_amp_px"], cfg["glitch_height_frac"])
