"""tests/shard_model.py (the host model tests/test_shard_fixup_gpu.py holds the commit and shard fix-up kernels to, bit for bit) tied to what
the suite already trusts.  CPU only.

  * its fix-up equals tests/test_shard_gloo.OracleEngine.correct, the engine the world 2 / 3 / 8 gloo runs validated against the in-order render;
  * math.pow (the model's coefficient) equals libm's pow (the library's) for every persistence the GPU tests use and k = 1 .. 200;
  * its commit equals commit_pixel<float>'s expressions written out: clip(f32(p) * state + f32(1 - p) * static) and
    fma(state, f32(p), static * f32(1 - p));
  * DESIGN.md §7's linearity claim, on the very clips the GPU end-to-end tests run: the sharded protocol against the in-order render;
  * include/crtfx.h's prototypes of the three entries against _lib.py's ctypes signatures, argument by argument."""
import ctypes
import ctypes.util
import math
import os
import re

import numpy as np
import pytest
import torch

from pythoncrt_amd import _lib
from pythoncrt_amd.shard import FrameShard, ShardedRender, settle_frames
from tests import shard_model as sm
from tests import warp_model as wm
from tests.test_shard_gloo import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def libm():
    return ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")


@pytest.mark.parametrize("p", sm.PERSISTENCE)
def test_fixup_is_the_gloo_tests_engine(p):
    """26 frames of the kernel tests' inputs (ties, both clips) through OracleEngine.correct and through fixup + to_u8."""
    h, w, n = 7, 63, 26
    carry = sm.make_carry(h, w, 12)
    local = sm.make_locals(n, h, w, 11, carry)
    out = torch.zeros((n, h, w, 3), dtype=torch.uint8)
    OracleEngine(p).correct(torch.from_numpy(local), torch.from_numpy(carry), p, out)
    for j in range(n):
        assert np.array_equal(out[j].numpy(), wm.to_u8(sm.fixup(local[j], carry, p, j + 1))), j


def test_math_pow_is_the_librarys_pow():
    """The library narrows libm's pow(p, (double)k); the model narrows math.pow(p, k) — and ShardedRender's own `p ** n` is the same double."""
    m = libm()
    m.pow.restype = ctypes.c_double
    m.pow.argtypes = [ctypes.c_double, ctypes.c_double]
    for p in sm.PERSISTENCE:
        for k in range(1, 201):
            assert math.pow(p, k) == m.pow(p, float(k)) == p ** k, (p, k)
    # where the coefficients leave the normal range (the deep-power case of the GPU test)
    assert sm.coeff(0.5, 126) == np.float32(2.0 ** -126) and 0.0 < sm.coeff(0.5, sm.DEEP_POWER) < np.finfo(np.float32).tiny
    assert sm.coeff(0.5, 149) > 0.0 and sm.coeff(0.5, 150) == 0.0


@pytest.mark.parametrize("p", sm.PERSISTENCE)
def test_commit_is_commit_pixels_arithmetic(p):
    """commit() goes through orc.persistence_blend / orc.add_weighted (render_chain / preview_step); here commit_pixel<float>'s expressions are
    written out in float32, the fused one with libm's fmaf."""
    m = libm()
    m.fmaf.restype = ctypes.c_float
    m.fmaf.argtypes = [ctypes.c_float] * 3
    h, w = 7, 63
    static = sm.make_locals(1, h, w, 21)[0]
    static = np.clip(static, 0.0, 1.0)          # a static image lies in [0, 1]
    state = sm.make_carry(h, w, 22)
    pf, qf = np.float32(p), np.float32(1.0 - p)
    assert np.array_equal(sm.commit(static, state, sm.BLEND_NONE, p), static)
    assert np.array_equal(sm.commit(static, None, sm.BLEND_RENDER, p), static)
    render = np.clip(pf * state + qf * static, np.float32(0.0), np.float32(1.0))
    assert render.dtype == np.float32
    assert np.array_equal(sm.commit(static, state, sm.BLEND_RENDER, p), render)
    assert np.array_equal(sm.commit(static, state, sm.BLEND_RENDER, p), wm.render_chain([static], p, state)[0])
    prod = static * qf
    preview = np.array([m.fmaf(float(s), float(pf), float(t)) for s, t in zip(state.ravel(), prod.ravel())], np.float32).reshape(static.shape)
    assert np.array_equal(sm.commit(static, state, sm.BLEND_PREVIEW, p), preview)
    assert np.array_equal(sm.commit(static, state, sm.BLEND_PREVIEW, p), wm.preview_step(static, p, state)[1])
    # the fusion is visible on these inputs: the two-rounding form differs somewhere, so the check above tells the two apart
    # (p = 0.5: the product by 0.5 is exact and the two forms are one)
    assert np.array_equal(preview, pf * state + prod) == (p == 0.5)


def test_schedules_are_what_the_engine_and_the_protocol_derive():
    """keep = min(chunk, settle_frames(p, 2 ** -26)) (GpuShardEngine, run_round, _finish); the carry rule is ShardedRender.parallel_hop."""
    for p, chunk, keep in sm.SCHEDULES:
        assert keep == min(chunk, settle_frames(p, 2.0 ** -26)), (p, chunk)
        assert (sm.schedule_rule(p, chunk) == "parallel") == ShardedRender(FrameShard(2, 0, chunk), p, engine=None).parallel_hop
    assert [sm.schedule_rule(p, c) for p, c, _ in sm.SCHEDULES] == ["exact", "parallel", "parallel"]
    assert any(k < c for _, c, k in sm.SCHEDULES) and any(k == c for _, c, k in sm.SCHEDULES)      # a capped chunk and an uncapped one
    assert sm.LONG_COUNTS == (sm.HALO_MAX_FRAMES, sm.HALO_MAX_FRAMES + 1, 2 * sm.HALO_MAX_FRAMES + 2)


def test_kernel_inputs_reach_both_clips_and_the_ties():
    """On every shape of the kernel tests, over the frames it runs, the drawn inputs are finite and (from 3 x 5 up) push corrected sums past 1 and
    below 0; the tie values survive a zero carry."""
    for h, w in sm.SHAPES:
        n = 130 if (h, w) in sm.SMALL else 26
        carry = sm.make_carry(h, w, 100 * h + w + 1)
        local = sm.make_locals(n, h, w, 100 * h + w, carry)          # the batch test's own draw
        assert np.isfinite(local).all() and np.isfinite(carry).all() and carry.min() >= 0.0 and carry.max() <= 1.0
        if h * w == 1:
            continue
        for p in sm.PERSISTENCE:
            raw = local[:2] + sm.coeff(p, 1) * carry
            assert (raw > 1.0).any() and (raw < 0.0).any(), (h, w, p)
        assert (carry == 0.0).any() and (carry == 1.0).any()
    t = sm._ties_u8(np.random.default_rng(0), 4096)
    s = t * np.float32(255.0)
    assert (s - np.floor(s) == 0.5).sum() > 200                       # exact ties of the uint8 quantiser
    th = sm._ties_half(np.random.default_rng(0), 4096) * np.float32(255.0)
    back = th.astype(np.float16).astype(np.float32)
    assert (np.abs(th - back) == sm_half_ulp(th) * 0.5).sum() > 200      # exact ties of the narrowing to half


def sm_half_ulp(x):
    """Spacing of float16 at |x| (normal range)."""
    x = np.maximum(np.abs(np.asarray(x, np.float32)), np.float32(2.0 ** -14))
    return np.exp2(np.floor(np.log2(x)) - 10.0)


@pytest.mark.parametrize("half", [False, True], ids=["u8", "half"])
@pytest.mark.parametrize("name", sorted(sm.SETTINGS))
def test_sharded_model_within_the_in_order_bar(name, half):
    """state_t = local_t + p^(t - t0 + 1) * carry.  The sharded protocol under the model against the in-order render under the model, on
    every clip of the GPU end-to-end tests (both shapes, the three schedules, three chunks each).  Each case alone must meet the project's
    bar: uint8 frames within 1 LSB on < 1e-3 of the samples, half frames within one half ulp on < 1e-3 of the samples.
    Measured (largest share of differing samples over the six cases of a setting; u8 / half):
        off 7.2e-6 / 2.4e-5, vig 1.8e-6 / 2.5e-5, bloom32 6.0e-6 / 2.4e-5, bloom64 6.0e-6 / 1.8e-5, point 6.0e-6 / 4.3e-5
    — at most 4 uint8 samples (1 LSB) and 26 half samples (one half ulp) of a clip of up to 1.1 M samples; run with -s for every case's count."""
    worst = 0.0
    for h, w in sm.E2E_SHAPES:
        for p, chunk, keep in sm.SCHEDULES:
            cfg, point = sm.e2e_cfg(name, p)
            frames = sm.clip(h, w, half, sm.E2E_CHUNKS * chunk)
            got, _ = sm.sharded(frames, cfg, half, chunk, keep, sm.schedule_rule(p, chunk), sm.E2E_FIRST, point)
            exp, _ = sm.in_order(frames, cfg, half, sm.E2E_FIRST, point)
            got, exp = np.stack(got), np.stack(exp)
            if half:
                d = np.abs(got.astype(np.float32) - exp.astype(np.float32))
                assert np.all(d <= sm_half_ulp(exp)), (h, w, p, chunk)
            else:
                d = np.abs(got.astype(np.int16) - exp.astype(np.int16))
                assert d.max() <= 1, (h, w, p, chunk)
            share = float((d != 0).mean())
            print(f"{name} {'half' if half else 'u8'} {h}x{w} p={p} chunk={chunk}: {int((d != 0).sum())} of {d.size} differ ({share:.2e})")
            assert share < 1e-3, (h, w, p, chunk, share)
            worst = max(worst, share)
    print(f"{name} {'half' if half else 'u8'}: worst share {worst:.2e}")


C_TYPES = {"int": ctypes.c_int, "double": ctypes.c_double, "size_t": ctypes.c_size_t}


def test_header_prototypes_of_the_three_entries():
    """include/crtfx.h against _lib.SYMBOLS for crtfx_blend_quantise, crtfx_halo_correct_quantise and crtfx_halo_correct_batch: the argument
    count, and the kind of every argument in order (any pointer: c_void_p; int, double, size_t: themselves) — a swapped pair of
    (double, pointer) or (int, size_t) arguments would pass a count check."""
    hdr = open(os.path.join(ROOT, "include", "crtfx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = {"crtfx_blend_quantise": ["ctx", "static_dev", "state_inout_dev", "out_pix_dev", "blend", "persistence", "stream"],
             "crtfx_halo_correct_quantise": ["ctx", "local_dev", "carry_in_dev", "coeff", "state_out_dev", "out_pix_dev", "stream"],
             "crtfx_halo_correct_batch": ["ctx", "local_base_dev", "carry_in_dev", "persistence", "first_power", "n", "out_base", "out_stride_bytes",
                                          "stream"]}
    for name, want in names.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        res, sig = _lib.SYMBOLS[name]
        assert res is ctypes.c_int and len(args) == len(sig) == len(want), (name, args)
        for a, ct, nm in zip(args, sig, want):
            assert a.split()[-1].lstrip("*") == nm, (name, a, nm)      # the order the tests and pipeline.py pass them in
            kind = ctypes.c_void_p if "*" in a else C_TYPES[a.split()[-2]]
            assert ct is kind, (name, a, ct)
