"""The host model of the frame-sharded persistence path: what k_commit (crtfx_blend_quantise, crtfx_halo_correct_quantise),
k_halo_batch (crtfx_halo_correct_batch) and GpuShardEngine.local_scan / correct behind shard.ShardedRender must produce, bit for bit.

It restates the arithmetic of crtfx_warp.hip.h's k_commit / k_halo_batch and crtfx_common.hip.h's commit_pixel<float> and takes everything
else from tests/warp_model.py (the effect chain, the in-order commit, the two quantisers):

  * coefficient: the library computes (float)pow(persistence, (double)k) on the host; math.pow is the same libm call (tests/test_shard_model.py
    holds the two together for every p and k the GPU tests use);
  * fix-up: clip(local + coeff * carry) in float32 — the product is rounded, then the sum (the library is built with -ffp-contract=off) —
    and quantised with warp_model.to_u8 / to_half;
  * commit (mode 0 of k_commit): orc.persistence_blend / orc.add_weighted on float32 inputs, as warp_model.render_chain / preview_step
    apply them, so the model adds no arithmetic of its own; q is the double difference narrowed, float32(1.0 - p);
  * local scan: warp_model.render (point_render for the pointwise chain) from no state at the start of the clip and from an all-zero float32
    state anywhere else;
  * the protocol: per chunk a local scan, then the fix-up of its first min(n, keep) frames with the carry; the frames behind `keep` keep the
    bytes of the scan.  The carry follows shard.ShardedRender: "parallel" (run_round's parallel hop and _finish: every rank forwards its
    chunk-final LOCAL state, so chunk c is corrected with the local final of chunk c - 1) or "exact" (the chain: the TRUE final travels,
    true_c = local_final_c + float32(p ** n) * true_{c-1}, a float32 product and a float32 sum without a clip, as torch evaluates
    `final_local + (p ** n) * carry`; the first chunk's local final is its true one).

Inputs must be finite: np.clip and fminf(fmaxf()) differ on NaN.

Only numpy and the oracle: nothing here imports torch or the package."""
import math

import numpy as np

from tests import point_builds as pb
from tests import warp_model as wm

BLEND_NONE, BLEND_RENDER, BLEND_PREVIEW = 0, 1, 2      # CRTFX_BLEND_* of include/crtfx.h
HALO_MAX_FRAMES = 64                                   # frames per k_halo_batch launch (crtfx_warp.hip.h)


def coeff(p, k):
    """The float32 coefficient of frame k of a chunk (k = 1 for its first frame)."""
    return np.float32(math.pow(float(p), int(k)))


def fixup_coeff(local32, carry32, c32):
    assert local32.dtype == np.float32 and carry32.dtype == np.float32 and type(c32) is np.float32
    prod = c32 * carry32
    assert prod.dtype == np.float32
    return np.clip(local32 + prod, np.float32(0.0), np.float32(1.0))


def fixup(local32, carry32, p, k):
    """The corrected float32 state of one frame: clip(local + coeff(p, k) * carry)."""
    return fixup_coeff(local32, carry32, coeff(p, k))


def commit(static32, state32, blend, p):
    """k_commit mode 0 = commit_pixel<float>: the float32 state after one crtfx_blend_quantise call."""
    assert static32.dtype == np.float32 and (state32 is None or state32.dtype == np.float32)
    if blend == BLEND_NONE:
        return static32.copy()
    if blend == BLEND_RENDER:
        return wm.render_chain([static32], p, state32)[0]
    assert blend == BLEND_PREVIEW
    return wm.preview_step(static32, p, state32)[1]


def _render(point):
    return wm.point_render if point else wm.render


def local_scan(frames, cfg, half, first, clip_start, point=False):
    """A chunk as a rank scans it alone -> (uncorrected frames, every local float32 state)."""
    h, w = frames[0].shape[:2]
    state = None if clip_start else np.zeros((h, w, 3), np.float32)
    return _render(point)(frames, cfg, half, first=first, state=state)


def in_order(frames, cfg, half, first=0, point=False):
    """The single-process render of the whole clip -> (frames, states)."""
    return _render(point)(frames, cfg, half, first=first)


def sharded(frames, cfg, half, chunk, keep, rule, first=0, point=False):
    """The whole protocol on one host -> (frames, the carry every chunk was corrected with (None for the first))."""
    assert rule in ("parallel", "exact")
    p = cfg["persistence"]
    out, carries = [], []
    prev = None                                        # what the previous chunk sent on
    for lo in range(0, len(frames), chunk):
        part = frames[lo:lo + chunk]
        n = len(part)
        scanned, local = local_scan(part, cfg, half, first + lo, clip_start=(lo == 0), point=point)
        carry = prev
        carries.append(carry)
        if carry is not None:
            for j in range(min(n, keep)):
                scanned[j] = wm.quantise(fixup(local[j], carry, p, j + 1), half)
        if rule == "parallel" or carry is None:
            prev = local[-1]
        else:
            prev = local[-1] + np.float32(p ** n) * carry
            assert prev.dtype == np.float32
        out += scanned
    return out, carries


# ---- the inputs of the kernel tests ----------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (3, 5), (4, 64), (5, 65), (7, 63), (9, 127), (6, 128), (33, 130), (13, 191))
SMALL = SHAPES[:3]                                     # the shapes that also run the chunks of more than one launch
PERSISTENCE = (0.2, 0.5, 0.97)
COUNTS = (0, 1, 2, 26)
LONG_COUNTS = (64, 65, 130)                            # one full launch, one frame into the second, two frames into the third
FIRST_POWERS = (1, 3)
DEEP_POWER = 127                                       # p = 0.5: float32(0.5 ** k) is subnormal from k = 127 and zero from k = 150


def _ties_u8(rng, size):
    """k / 255 and (k + 0.5) / 255 (the quantiser's ties) and their float32 neighbours on either side."""
    k = rng.integers(0, 256, size).astype(np.float32)
    v = ((k + np.float32(0.5) * rng.integers(0, 2, size).astype(np.float32)) / np.float32(255.0)).astype(np.float32)
    step = rng.integers(-1, 2, size)
    v = np.where(step < 0, np.nextafter(v, np.float32(-1.0)), np.where(step > 0, np.nextafter(v, np.float32(2.0)), v))
    return np.minimum(v, np.float32(1.0)).astype(np.float32)


def _ties_half(rng, size):
    """Values whose float32 product with 255 lands on or next to the midpoint of two neighbouring halves."""
    bits = rng.integers(0x0400, 0x5BF8, size).astype(np.uint16)          # positive normal halves below 255
    lo = bits.view(np.float16).astype(np.float32)
    hi = (bits + np.uint16(1)).view(np.float16).astype(np.float32)
    v = ((lo + hi) * np.float32(0.5) / np.float32(255.0)).astype(np.float32)
    step = rng.integers(-1, 2, size)
    return np.where(step < 0, np.nextafter(v, np.float32(-1.0)), np.where(step > 0, np.nextafter(v, np.float32(2.0)), v)).astype(np.float32)


def make_carry(h, w, seed):
    """A float32 carry frame: uniform values with full mantissas, salted with exact 0 (the local value then passes through: the ties below
    reach the quantiser as drawn) and exact 1 (the largest correction)."""
    rng = np.random.default_rng(seed)
    c = rng.random((h, w, 3), dtype=np.float32)
    kind = rng.integers(0, 10, c.shape)
    c[kind < 3] = 0.0
    c[kind == 9] = 1.0
    return c


TUNED = ((0.97, False), (0.2, False), (0.2, True))      # (p, half): the coefficients and the quantiser a share of make_locals' values is aimed at


def _aimed(rng, shape, carry, p, half, powers):
    """Local values that leave frame j's corrected sum — coefficient p ** powers[j] on this very carry — on a quantiser tie or within an ulp
    or two of one: local = tie - float32(coeff * carry).  There the product's own rounding decides the sample, so a fix-up that contracts
    the product and the sum into one fma, or takes a neighbouring coefficient, changes pixels and not only the last bit of a state."""
    out = np.empty(shape, np.float32)
    for j in range(shape[0]):
        tie = (_ties_half if half else _ties_u8)(rng, shape[1:])
        out[j] = tie - coeff(p, powers[j]) * carry
    return out


def make_locals(n, h, w, seed, carry=None, powers=None):
    """n float32 local-state frames: uniform [0, 1]; exact 0 and 1; quantiser ties of both pixel formats and their neighbours; values close to 1
    (the corrected sum passes 1: the upper clip) and slightly negative ones (the lower clip); with a carry, values aimed at the ties of the
    corrected sum (_aimed; frame j is corrected with p ** powers[j], default j + 1).  Finite throughout."""
    rng = np.random.default_rng(seed)
    shape = (n, h, w, 3)
    v = rng.random(shape, dtype=np.float32)
    kind = rng.integers(0, 12, shape)
    v = np.where(kind == 0, np.float32(0.0), v)
    v = np.where(kind == 1, np.float32(1.0), v)
    v = np.where((kind == 2) | (kind == 3), _ties_u8(rng, shape), v)
    v = np.where(kind == 4, _ties_half(rng, shape), v)
    v = np.where(kind == 5, np.float32(1.0) - rng.random(shape, dtype=np.float32) * np.float32(0.05), v)
    v = np.where(kind == 6, -rng.random(shape, dtype=np.float32) * np.float32(1e-3), v)
    if carry is not None:
        powers = list(range(1, n + 1)) if powers is None else list(powers)
        for i, (p, half) in enumerate(TUNED):
            v = np.where(kind == 7 + i, _aimed(rng, shape, carry, p, half, powers), v)
    v = np.ascontiguousarray(v, np.float32)
    assert np.isfinite(v).all()
    return v


# ---- the inputs of the engine tests (GPU) and of the linearity bound (CPU): the same clips ------------------------------------------------
WARP = 0.15
SETTINGS = {"off": (dict(wm.OFF, warp_strength=WARP), False), "vig": (dict(wm.VIG, warp_strength=WARP), False),
            "bloom32": (dict(wm.BLOOM32, warp_strength=WARP), False), "bloom64": (dict(wm.BLOOM64, warp_strength=WARP), False),
            "point": (dict(pb.DEFAULTS, noise_strength=0.0), True)}      # name -> (settings, pointwise chain)
E2E_SHAPES = ((48, 64), (37, 70))
SCHEDULES = ((0.5, 6, 6), (0.5, 40, 26), (0.2, 16, 12))      # (persistence, chunk, keep = min(chunk, settle_frames(p, 2 ** -26)))
E2E_FIRST = 0
E2E_CHUNKS = 3                                                # a clip start, a corrected chunk, and one corrected behind a corrected one


def schedule_rule(p, chunk):
    """ShardedRender.parallel_hop restated: one parallel hop per round once p ** chunk is below float32 resolution, else the exact chain."""
    return "parallel" if (p ** chunk) < 2.0 ** -24 else "exact"


def clip(h, w, half, n):
    return [wm.make_frame(h, w, 9000 + 31 * h + w + j, half) for j in range(n)]


def e2e_cfg(name, p):
    cfg, point = SETTINGS[name]
    return dict(cfg, persistence=p), point
