"""CPU: the walks of tests/ctx_transitions.py can see a stale read.

  * Tables: across every same-table arrow the two stops upload host tables of the same byte size and different content (a kernel that read
    the old one would read without a fault); where one stop uploads nothing the other's table exists.
  * Images: across every step of every walk the oracle's float image of the two stops differs in >= 5 % of the samples and the quantised
    uint8 image in >= 1 % — conditions on the inputs, not tolerances on the kernels.
  * Coverage: every stop is in the star walk, every arrow in the pairs walk in both directions, the random walk is seeded by literals, and
    every family prefix of the table exists among the library's kernels."""
import os
import sys

import numpy as np
import pytest

from oracle import crt_oracle as orc
from tests import ctx_transitions as ct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOAT_SHARE, U8_SHARE = 0.05, 0.01


def host_tables(stop, h, w, pix):
    """The host tables Engine.set_params uploads for a stop, by kind (restated from pythoncrt_amd/effects.py with pythoncrt_amd.tables)."""
    from pythoncrt_amd import _lib, tables
    c = stop.config()
    out = {}
    per_channel = c["temperature"] != 0.0 or c["brightness"] != 0.0 or c["contrast"] != 1.0 or (c["gamma"] != 1.0 and c["gamma"] > 0.0)
    if pix == "u8" and c["saturation"] == 1.0 and per_channel:
        out["grade_lut"] = (tables.grade_lut(c["brightness"], c["contrast"], c["gamma"], c["temperature"]),)
    if c["pixel_size"] > 1:
        out["pixelate"] = tables.pixelate_maps(h, w, c["pixel_size"])
    if c["bloom_strength"] > 0.0 and c["bloom_sigma"] > 0.0 and not c["fast_bloom"]:
        k = tables.bloom_ksize(c["bloom_sigma"])
        out["taps"] = (tables.gaussian_taps(k, c["bloom_sigma"]),)
    if c["triad_strength"] > 0.0 and not stop.settings.get("_planes"):
        out["triad_row"] = (tables.triad_row(_lib.load(), w, c["triad_strength"], c["triad_softness"]),)
        if tables.triad_uses_lut(c["triad_gamma"], c["triad_preserve_luma"]):
            out["triad_luts"] = tables.triad_luts(c["triad_gamma"])
    if c["noise_strength"] > 0.0 and c["grain_size"] > 1:
        gh, gw = max(1, h // c["grain_size"]), max(1, w // c["grain_size"])
        out["grain_axes"] = tables.resize_linear_axis(w, gw) + tables.resize_linear_axis(h, gh)
    if c["warp_strength"] != 0.0:
        xhat, yhat, cx, cy = tables.warp_axes(h, w)
        out["warp_scalars"] = (np.array([float(c["warp_strength"]) * 0.5, cx, cy]),)
    return {k: tuple(np.ascontiguousarray(a) for a in v) for k, v in out.items()}


@pytest.mark.parametrize("size", list(ct.SIZES))
def test_same_table_arrows_swap_tables_of_one_size(size):
    h, w = ct.SIZES[size]
    n_same = n_drop = 0
    for ar in ct.ARROWS:
        for pix in ar.pix:
            ta, tb = host_tables(ct.BY_NAME[ar.a], h, w, pix), host_tables(ct.BY_NAME[ar.b], h, w, pix)
            for kind in ar.same:
                assert kind in ta and kind in tb, (ar, kind)
                assert [a.nbytes for a in ta[kind]] == [b.nbytes for b in tb[kind]], (ar, kind, "byte sizes differ")
                assert any(not np.array_equal(a, b) for a, b in zip(ta[kind], tb[kind])), (ar, kind, "same content")
                n_same += 1
            for kind in ar.drops:
                assert kind in ta and ta[kind][0].nbytes > 0 and kind not in tb, (ar, kind)
                n_drop += 1
    assert n_same >= 9 and n_drop >= 8
    # the radii the table's notes claim
    from pythoncrt_amd import tables
    radius = lambda s: (tables.bloom_ksize(ct.BY_NAME[s].config()["bloom_sigma"]) - 1) // 2
    assert [radius(s) for s in ("taps_0p9", "taps_1p1", "taps_2p9", "taps_3p1", "taps_5p5", "taps_11p0", "taps_11p1", "taps_20", "full")] == \
        [3, 3, 9, 9, 16, 33, 33, 60, 9]


_IMAGES = {}


def oracle_image(name, size):
    """The oracle's float image of a stop on the test frame, and its quantised uint8 image."""
    key = (name, size)
    if key not in _IMAGES:
        stop = ct.BY_NAME[name]
        h, w = ct.SIZES[size]
        cfg = stop.config()
        g = cfg["grain_size"]
        plane = np.random.default_rng(77).standard_normal((max(1, h // g), max(1, w // g)) if g > 1 else (h, w), dtype=np.float32)
        img = orc.apply_static_effects(*ct.static_args(ct.make_frame(h, w, 3), ct.api_masks(orc, stop, h, w), cfg),
                                       time_sec=ct.TIME_SEC, noise_plane=plane if cfg["noise_strength"] > 0.0 else None, **ct.api_keywords(stop, h, w))
        _IMAGES[key] = (img.astype(np.float32), orc.convert_scale_abs(np.ascontiguousarray(img), 255.0))
    return _IMAGES[key]


def all_steps():
    out = {}
    for route in ct.ROUTES:
        for pix in ct.PIXES:
            for wname, walk in ct.WALKS.items():
                for a, b in ct.steps(walk(route, pix)):
                    out.setdefault(frozenset((a, b)), (a, b, route, wname))
    return out


@pytest.mark.parametrize("size", list(ct.SIZES))
def test_every_step_changes_the_picture(size):
    bad = []
    tight = (1.0, 1.0, None)
    for a, b, route, wname in all_steps().values():
        (fa, ua), (fb, ub) = oracle_image(a, size), oracle_image(b, size)
        fs, us = float((fa != fb).mean()), float((ua != ub).mean())
        if us < tight[1]:
            tight = (fs, us, (a, b))
        if fs < FLOAT_SHARE or us < U8_SHARE:
            bad.append(f"{a} -> {b} ({route}, {wname}): float share {fs:.4f}, u8 share {us:.4f}")
    print(f"{size}: {len(all_steps())} distinct steps; the tightest is {tight[2]}: float {tight[0]:.4f}, u8 {tight[1]:.4f}")
    assert not bad, "\n".join(bad)


def test_walks_cover_the_table():
    for route in ct.ROUTES:
        for pix in ct.PIXES:
            names = ct.stops_of(route, pix)
            star = ct.star_walk(route, pix)
            assert set(names) <= set(star) and all("full" in st for st in ct.steps(star))
            st = set(ct.steps(ct.pairs_walk(route, pix)))
            for ar in ct.ARROWS:
                if ar.a in names and ar.b in names:
                    assert (ar.a, ar.b) in st and (ar.b, ar.a) in st, ar
            rnd = ct.random_walk(route, pix)
            assert len(ct.steps(rnd)) == ct.RANDOM_STEPS == 40 and rnd == ct.random_walk(route, pix) and set(rnd) <= set(names)
            assert all(a != b for w in (star, ct.pairs_walk(route, pix), rnd) for a, b in ct.steps(w))
    assert (ct.RANDOM_SEED, ct.RANDOM_STEPS) == (20260, 40)
    # every stop belongs to a route and every arrow joins stops of the table; the groups the table must hold are there
    assert all(ar.a in ct.BY_NAME and ar.b in ct.BY_NAME for ar in ct.ARROWS)
    assert {s.name for s in ct.STOPS} == {n for r in ct.ROUTES for p in ct.PIXES for n in ct.stops_of(r, p)}
    for h, w in ct.SIZES.values():
        assert h <= 64 and w <= 256
    assert ct.SIZES["even"][1] % 8 == 0 and ct.SIZES["even"][1] >= 128 and ct.SIZES["odd"][0] % 2 == 1 and ct.SIZES["odd"][1] % 2 == 1


def test_every_family_prefix_is_a_kernel_of_the_library():
    """Every prefix a stop must land on names at least one kernel of libcrtfx.so (tools/kernel_resources.resources)."""
    from pythoncrt_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources as kr
    finally:
        sys.path.pop(0)
    kernels = set(kr.resources(_lib.LIB_PATH))
    prefixes = {fam.split("=", 1)[1] for s in ct.STOPS for fam in s.family.values()}
    assert len(prefixes) >= 10
    for p in sorted(prefixes):
        # (k_warp is no template: its plan string k_warp<gather|commit-only> names a run-time argument)
        assert any(k.startswith("crtfx::" + p) or (p.endswith("<") and k == "crtfx::" + p[:-1]) for k in kernels), p
    keys = {fam.split("=", 1)[0] for s in ct.STOPS for fam in s.family.values()}
    assert keys <= {"phosphor", "point", "half", "warp", "blur"}
    # every pattern of a stop resolves for every (route, format, size) it runs on
    for s in ct.STOPS:
        for route in s.routes:
            for pix in s.pixes:
                for size in ct.SIZES:
                    key, prefix = s.family_for(route, pix, size)
                    assert key and prefix
