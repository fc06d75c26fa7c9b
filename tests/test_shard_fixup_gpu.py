"""The commit and shard fix-up kernels (k_commit, k_halo_batch) and the engine that feeds them (GpuShardEngine.local_scan / correct behind
shard.ShardedRender) held to tests/shard_model.py, bit for bit.

Everything these kernels do is deterministic float32 arithmetic (the library is built with -ffp-contract=off), so every comparison here is
np.array_equal against the host model — no sample allowance — and no GPU output feeds the model: local states, carries, static images and
frames are all drawn on the host.  tests/test_shard_model.py ties the model to the oracle engine of the gloo tests, to libm's pow and to
the in-order render (the linearity bound of DESIGN.md §7) on the CPU.

The kernel inputs (shard_model.make_locals / make_carry) are finite float32 values: uniform ones with full mantissas, exact 0 and 1, the
ties of both quantisers and their float32 neighbours (reaching the quantiser unchanged through a zero carry), sums that pass 1 and locals
below 0 (both clips), and locals aimed so that the corrected sum itself lands on a tie — there a contracted product-and-sum or a neighbouring
coefficient changes the pixel, not only the last bit of a state the batch entry never returns.

Kernels alone, on shard_model.SHAPES (1x1 .. 13x191: widths below, at and ragged against the 64-pixel tile, W % 4 in {0, 1, 2, 3} — the
uint8 row store takes its dword path only where a row starts 4-aligned, so the odd widths alternate paths row by row — heights that are
no multiple of the 4 rows of a block), uint8 and half frames on each:
  * crtfx_halo_correct_batch: p in {0.2, 0.5, 0.97} x first_power in {1, 3} x n in {0, 1, 2, 26} (and 64, 65, 130 — the split into launches
    of 64 frames — on the three smallest shapes) x an output stride of one frame and of a frame plus 16 bytes; one call at p = 0.5 from
    first_power 127 on, where float32(p ** k) is subnormal and then zero.  The output lies in a buffer pre-filled with a sentinel,
    with guard bytes on either side: every byte outside the n frames must keep the sentinel, and n = 0 writes nothing.
  * crtfx_halo_correct_quantise: the same frame as the batch call and the model; the float32 state; state alone and pixels alone.
  * crtfx_blend_quantise: NONE / RENDER / PREVIEW x the three p: the state in place, the pixels, a NULL pixel pointer, a chain of three calls
    against warp_model.render_chain / preview_step.
  * the host-side refusals: CRTFX_E_INVALID, a message, and no byte written.

The engine end to end, on shard_model.SETTINGS (the warp chain unpromoted, promoted, behind the Gaussian bloom in both dtypes; the
pointwise fast-bloom defaults) x uint8 / half x 48x64 and 37x70 x the schedules (p, chunk, keep) = (0.5, 6, 6), (0.5, 40, 26), (0.2, 16, 12):
a clip-start chunk, a chunk scanned from zero in each slot of a two-slot engine and corrected with a host-drawn carry (the frames behind `keep`
untouched), a three-round ShardedRender of one rank and a hand-run parallel-hop sequence of three chunks against shard_model.sharded."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import shard_model as sm  # noqa: E402
from tests import warp_model as wm  # noqa: E402

GUARD = 64                                  # bytes before and after the output frames
SENTINEL = 0xA5
STATE_SENTINEL = -7.0
PADS = (0, 16)                              # output stride = a frame + this many bytes
E_INVALID = -1

_PIPES = {}


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from pythoncrt_amd import effects
    saved = effects.DEBUG_OPTIONS
    effects.DEBUG_OPTIONS = {}
    yield effects
    effects.DEBUG_OPTIONS = saved
    _PIPES.clear()
    torch.cuda.empty_cache()


def device():
    return torch.device("cuda", torch.cuda.current_device())


def stream():
    return torch.cuda.current_stream(device()).cuda_stream


def render_settings(cfg):
    from pythoncrt_amd.pipeline import RenderSettings
    return RenderSettings(**cfg)


def ctx_pipe(h, w, half):
    """A FramePipeline whose ctx the kernel tests call into (one per shape and pixel format for the whole module)."""
    from pythoncrt_amd.pipeline import FramePipeline
    key = (h, w, half)
    if key not in _PIPES:
        _PIPES[key] = FramePipeline(device(), h, w, render_settings(wm.OFF), fps=30.0, noise_seed=1, dtype=torch.float16 if half else torch.uint8)
    return _PIPES[key]


def describe(got, exp, what):
    """None when equal; else a line that says how many samples differ, by how much and where first."""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.shape == exp.shape and got.dtype == exp.dtype and np.array_equal(got, exp):
        return None
    if got.shape != exp.shape or got.dtype != exp.dtype:
        return f"{what}: {got.dtype}{got.shape} against {exp.dtype}{exp.shape}"
    bad = np.argwhere(got != exp)
    d = np.abs(got.astype(np.float64) - exp.astype(np.float64))
    return f"{what}: {len(bad)} of {got.size} differ; max |d| = {d.max():.3e}; first at {bad[0].tolist()} (got {got[tuple(bad[0])]!r}, model {exp[tuple(bad[0])]!r})"


def last_error(pipe):
    return (pipe.lib.crtfx_last_error(pipe.engine.ctx) or b"").decode()


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device())


class Guarded:
    """n output frames at a byte stride of a frame + pad inside a sentinel-filled device buffer with GUARD bytes on either side."""

    def __init__(self, n, h, w, half, pad=0):
        self.n, self.shape, self.half = n, (h, w, 3), half
        self.frame_bytes = h * w * 3 * (2 if half else 1)
        self.stride = self.frame_bytes + pad
        self.buf = torch.full((GUARD + n * self.stride + GUARD,), SENTINEL, dtype=torch.uint8, device=device())
        self.ptr = self.buf.data_ptr() + GUARD

    def read(self):
        """-> (the n frames, how many bytes outside them lost the sentinel)."""
        torch.cuda.synchronize()
        raw = self.buf.cpu().numpy()
        inside = np.zeros(raw.size, bool)
        frames = []
        for j in range(self.n):
            lo = GUARD + j * self.stride
            inside[lo:lo + self.frame_bytes] = True
            b = raw[lo:lo + self.frame_bytes].copy()
            frames.append((b.view(np.float16) if self.half else b).reshape(self.shape))
        return frames, int((raw[~inside] != SENTINEL).sum())


def check_frames(bad, g, model, what):
    frames, dirty = g.read()
    if dirty:
        bad.append(f"{what}: {dirty} padding / guard bytes overwritten")
    for j, f in enumerate(frames):
        line = describe(f, model[j], f"{what} frame {j}")
        if line:
            bad.append(line)
            break


SHAPE_PIX = [(h, w, half) for h, w in sm.SHAPES for half in (False, True)]
SHAPE_IDS = [f"{h}x{w}-{'half' if half else 'u8'}" for h, w, half in SHAPE_PIX]


# ---- k_halo_batch ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,half", SHAPE_PIX, ids=SHAPE_IDS)
def test_halo_correct_batch_against_model(env, h, w, half):
    pipe = ctx_pipe(h, w, half)
    lib, ctx = pipe.lib, pipe.engine.ctx
    counts = sm.COUNTS + (sm.LONG_COUNTS if (h, w) in sm.SMALL else ())
    nmax = max(counts)
    carry = sm.make_carry(h, w, 100 * h + w + 1)
    local = sm.make_locals(nmax, h, w, 100 * h + w, carry)
    d_local, d_carry = up(local), up(carry)
    bad, calls = [], 0
    for p in sm.PERSISTENCE:
        for fp in sm.FIRST_POWERS + ((sm.DEEP_POWER,) if p == 0.5 else ()):
            model = [wm.quantise(sm.fixup(local[j], carry, p, fp + j), half) for j in range(nmax)]
            for n in (counts if fp != sm.DEEP_POWER else (26,)):
                for pad in PADS:
                    g = Guarded(n, h, w, half, pad)
                    rc = lib.crtfx_halo_correct_batch(ctx, d_local.data_ptr(), d_carry.data_ptr(), p, fp, n, g.ptr, g.stride, stream())
                    calls += 1
                    what = f"p={p} first_power={fp} n={n} pad={pad}"
                    if rc != 0:
                        bad.append(f"{what}: rc {rc} ({last_error(pipe)})")
                        continue
                    check_frames(bad, g, model, what)
    assert not bad, f"{h}x{w} {'half' if half else 'u8'}: {len(bad)} failures in {calls} calls:\n" + "\n".join(bad[:25])


# ---- k_commit mode 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,half", SHAPE_PIX, ids=SHAPE_IDS)
def test_halo_correct_quantise_against_model_and_batch(env, h, w, half):
    pipe = ctx_pipe(h, w, half)
    lib, ctx = pipe.lib, pipe.engine.ctx
    powers = (1, 3, 26)
    carry = sm.make_carry(h, w, 200 * h + w + 1)
    local = sm.make_locals(len(powers), h, w, 200 * h + w, carry, powers)
    d_local, d_carry = up(local), up(carry)
    bad = []
    for p in sm.PERSISTENCE:
        for j, k in enumerate(powers):
            c = math.pow(p, k)
            assert np.float32(c) >= np.finfo(np.float32).tiny          # normal range: the state comparison below is exact
            m_state = sm.fixup(local[j], carry, p, k)
            m_pix = wm.quantise(m_state, half)
            what = f"p={p} k={k}"
            # state and pixels
            g = Guarded(1, h, w, half)
            st = torch.full((h, w, 3), STATE_SENTINEL, dtype=torch.float32, device=device())
            rc = lib.crtfx_halo_correct_quantise(ctx, d_local[j].data_ptr(), d_carry.data_ptr(), c, st.data_ptr(), g.ptr, stream())
            assert rc == 0, (what, last_error(pipe))
            check_frames(bad, g, [m_pix], what + " both")
            bad.append(describe(st.cpu().numpy(), m_state, what + " both: state"))
            # state alone
            st = torch.full((h, w, 3), STATE_SENTINEL, dtype=torch.float32, device=device())
            rc = lib.crtfx_halo_correct_quantise(ctx, d_local[j].data_ptr(), d_carry.data_ptr(), c, st.data_ptr(), None, stream())
            assert rc == 0, (what, last_error(pipe))
            bad.append(describe(st.cpu().numpy(), m_state, what + " state alone"))
            # pixels alone
            g = Guarded(1, h, w, half)
            rc = lib.crtfx_halo_correct_quantise(ctx, d_local[j].data_ptr(), d_carry.data_ptr(), c, None, g.ptr, stream())
            assert rc == 0, (what, last_error(pipe))
            check_frames(bad, g, [m_pix], what + " pixels alone")
            # the batch entry on the same frame
            gb = Guarded(1, h, w, half)
            rc = lib.crtfx_halo_correct_batch(ctx, d_local[j].data_ptr(), d_carry.data_ptr(), p, k, 1, gb.ptr, gb.stride, stream())
            assert rc == 0, (what, last_error(pipe))
            bad.append(describe(gb.read()[0][0], g.read()[0][0], what + " batch against single"))
    bad = [b for b in bad if b]
    assert not bad, f"{h}x{w} {'half' if half else 'u8'}: {len(bad)} failures:\n" + "\n".join(bad[:25])


# ---- k_commit mode 0 ---------------------------------------------------------------------------------------------------------------------
def chain_model(statics, blend, p, state0):
    if blend == sm.BLEND_NONE:
        return [s.copy() for s in statics]
    if blend == sm.BLEND_RENDER:
        return wm.render_chain(list(statics), p, state0)
    out, st = [], state0
    for s in statics:
        _, st = wm.preview_step(s, p, st)
        out.append(st)
    return out


@pytest.mark.parametrize("h,w,half", SHAPE_PIX, ids=SHAPE_IDS)
def test_blend_quantise_against_model(env, h, w, half):
    pipe = ctx_pipe(h, w, half)
    lib, ctx = pipe.lib, pipe.engine.ctx
    statics = np.clip(sm.make_locals(3, h, w, 300 * h + w), np.float32(0.0), np.float32(1.0))      # a static image lies in [0, 1]
    state0 = sm.make_carry(h, w, 300 * h + w + 1)
    d_static = up(statics)
    bad = []
    for blend, bname in ((sm.BLEND_NONE, "none"), (sm.BLEND_RENDER, "render"), (sm.BLEND_PREVIEW, "preview")):
        for p in sm.PERSISTENCE:
            what = f"{bname} p={p}"
            m_states = chain_model(statics, blend, p, state0)
            bad.append(describe(m_states[0], sm.commit(statics[0], state0, blend, p), what + ": the model's two forms"))
            # three calls threaded through one state buffer
            st = up(state0)
            for i in range(3):
                g = Guarded(1, h, w, half)
                rc = lib.crtfx_blend_quantise(ctx, d_static[i].data_ptr(), st.data_ptr(), g.ptr, blend, p, stream())
                assert rc == 0, (what, last_error(pipe))
                got = st.cpu().numpy()
                bad.append(describe(got, m_states[i], f"{what} call {i}: state"))
                check_frames(bad, g, [wm.quantise(m_states[i], half)], f"{what} call {i}")
                bad.append(describe(g.read()[0][0], wm.quantise(got, half), f"{what} call {i}: pixels against its own state"))
            # no pixel output: the state is still updated
            st = up(state0)
            rc = lib.crtfx_blend_quantise(ctx, d_static[0].data_ptr(), st.data_ptr(), None, blend, p, stream())
            assert rc == 0, (what, last_error(pipe))
            bad.append(describe(st.cpu().numpy(), m_states[0], what + " without pixels: state"))
    bad = [b for b in bad if b]
    assert not bad, f"{h}x{w} {'half' if half else 'u8'}: {len(bad)} failures:\n" + "\n".join(bad[:25])


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["u8", "half"])
def test_bad_arguments_are_refused_before_any_launch(env, half):
    h, w = 5, 65
    pipe = ctx_pipe(h, w, half)
    lib, ctx = pipe.lib, pipe.engine.ctx
    local, carry = up(sm.make_locals(2, h, w, 1)), up(sm.make_carry(h, w, 2))
    g = Guarded(2, h, w, half)
    st = torch.full((h, w, 3), STATE_SENTINEL, dtype=torch.float32, device=device())
    L, C, S, O, s = local.data_ptr(), carry.data_ptr(), st.data_ptr(), g.ptr, stream()
    nan = float("nan")
    calls = [("unknown blend", "blend mode", lambda: lib.crtfx_blend_quantise(ctx, L, S, O, 7, 0.5, s)),
             ("unknown blend -1", "blend mode", lambda: lib.crtfx_blend_quantise(ctx, L, S, O, -1, 0.5, s)),
             ("render without a state", "state_inout_dev", lambda: lib.crtfx_blend_quantise(ctx, L, None, O, sm.BLEND_RENDER, 0.5, s)),
             ("preview without a state", "state_inout_dev", lambda: lib.crtfx_blend_quantise(ctx, L, None, O, sm.BLEND_PREVIEW, 0.5, s)),
             ("blend NULL static_dev", "static_dev", lambda: lib.crtfx_blend_quantise(ctx, None, S, O, sm.BLEND_RENDER, 0.5, s)),
             ("single NULL local_dev", "NULL", lambda: lib.crtfx_halo_correct_quantise(ctx, None, C, 0.5, S, O, s)),
             ("single NULL carry_in_dev", "NULL", lambda: lib.crtfx_halo_correct_quantise(ctx, L, None, 0.5, S, O, s)),
             ("batch NULL local_base_dev", "halo batch", lambda: lib.crtfx_halo_correct_batch(ctx, None, C, 0.5, 1, 2, O, g.stride, s)),
             ("batch NULL carry_in_dev", "halo batch", lambda: lib.crtfx_halo_correct_batch(ctx, L, None, 0.5, 1, 2, O, g.stride, s)),
             ("batch n < 0", "halo batch", lambda: lib.crtfx_halo_correct_batch(ctx, L, C, 0.5, 1, -1, O, g.stride, s)),
             ("batch first_power 0", "halo batch", lambda: lib.crtfx_halo_correct_batch(ctx, L, C, 0.5, 0, 2, O, g.stride, s)),
             ("batch first_power -3", "halo batch", lambda: lib.crtfx_halo_correct_batch(ctx, L, C, 0.5, -3, 2, O, g.stride, s))]
    for p in (0.0, 1.0, -0.5, 1.5, nan):
        calls.append((f"render p={p}", "outside (0,1)", lambda p=p: lib.crtfx_blend_quantise(ctx, L, S, O, sm.BLEND_RENDER, p, s)))
        calls.append((f"preview p={p}", "outside (0,1)", lambda p=p: lib.crtfx_blend_quantise(ctx, L, S, O, sm.BLEND_PREVIEW, p, s)))
        calls.append((f"batch p={p}", "outside (0,1)", lambda p=p: lib.crtfx_halo_correct_batch(ctx, L, C, p, 1, 2, O, g.stride, s)))
    bad = []
    calls.append(("batch NULL out_base", "halo batch", lambda: lib.crtfx_halo_correct_batch(ctx, L, C, 0.5, 1, 2, None, g.stride, s)))
    for what, fragment, call in calls:
        assert lib.crtfx_halo_correct_batch(ctx, L, C, 0.5, 1, 0, O, g.stride, s) == 0      # a call that succeeds (n = 0: no launch) in between
        rc = call()
        msg = last_error(pipe)
        if rc != E_INVALID or fragment not in msg:      # the message of THIS refusal, not one left over from the call before
            bad.append(f"{what}: rc {rc}, message {msg!r}")
    frames, dirty = g.read()
    if dirty or any((f.view(np.uint8) != SENTINEL).any() for f in frames):
        bad.append("a refused call wrote pixels")
    if (st.cpu().numpy() != np.float32(STATE_SENTINEL)).any():
        bad.append("a refused call wrote the state")
    assert not bad, "\n".join(bad)


# ---- the engine end to end -----------------------------------------------------------------------------------------------------------
E2E = [(name, half) for name in sorted(sm.SETTINGS) for half in (False, True)]
E2E_IDS = [f"{name}-{'half' if half else 'u8'}" for name, half in E2E]


def engine_for(name, half, h, w, p, chunk, keep):
    from pythoncrt_amd.pipeline import FramePipeline, GpuShardEngine
    cfg, point = sm.e2e_cfg(name, p)
    pipe = FramePipeline(device(), h, w, render_settings(cfg), fps=30.0, noise_seed=1, dtype=torch.float16 if half else torch.uint8)
    eng = GpuShardEngine(pipe, chunk, slots=2)
    assert eng.keep == keep and eng.slots == 2
    return cfg, point, eng


def scan_lines(loc, out, m_out, m_states, keep, what):
    """The mismatch lines of one local scan: uncorrected frames, the kept local states and the chunk-final state."""
    n = len(m_out)
    k = min(n, keep)
    got_out, got_loc, got_final = out.cpu().numpy(), loc[:k].cpu().numpy(), loc[n - 1].cpu().numpy()
    lines = [describe(got_out[j], m_out[j], f"{what} frame {j}") for j in range(n)]
    lines += [describe(got_loc[j], m_states[j], f"{what} local state {j}") for j in range(k)]
    lines.append(describe(got_final, m_states[-1], f"{what} chunk-final state"))
    return [x for x in lines if x][:4]


@pytest.mark.parametrize("name,half", E2E, ids=E2E_IDS)
def test_engine_scan_and_correct_against_model(env, name, half):
    bad = []
    for h, w in sm.E2E_SHAPES:
        for p, chunk, keep in sm.SCHEDULES:
            cfg, point, eng = engine_for(name, half, h, w, p, chunk, keep)
            frames = sm.clip(h, w, half, 2 * chunk)
            d_frames = up(np.stack(frames))
            tag = f"{h}x{w} p={p} chunk={chunk}"
            # the first chunk of the clip: the in-order render outright
            m_out, m_states = sm.in_order(frames[:chunk], cfg, half, sm.E2E_FIRST, point)
            loc, out = eng.local_scan(d_frames[:chunk], sm.E2E_FIRST, clip_start=True, slot=0)
            bad += scan_lines(loc, out, m_out, m_states, keep, tag + " clip start:")
            # a later chunk: scanned from zero, then corrected with a host-drawn carry — in either slot
            m_out, m_states = sm.local_scan(frames[chunk:], cfg, half, sm.E2E_FIRST + chunk, clip_start=False, point=point)
            carry = wm.make_state(h, w, 17 * h + w)
            m_fixed = [wm.quantise(sm.fixup(m_states[j], carry, p, j + 1), half) for j in range(keep)] + m_out[keep:]
            assert any(not np.array_equal(a, b) for a, b in zip(m_fixed[:keep], m_out[:keep]))      # the fix-up changes the frames
            d_carry = up(carry)
            for slot in (0, 1):
                loc, out = eng.local_scan(d_frames[chunk:], sm.E2E_FIRST + chunk, clip_start=False, slot=slot)
                assert out.data_ptr() == eng.out_slots[slot].data_ptr()
                bad += scan_lines(loc, out, m_out, m_states, keep, f"{tag} slot {slot} scan:")
                eng.correct(loc[:keep], d_carry, p, out[:keep])
                got = out.cpu().numpy()
                lines = [describe(got[j], m_fixed[j], f"{tag} slot {slot} {'corrected' if j < keep else 'left as scanned'} frame {j}") for j in range(chunk)]
                bad += [x for x in lines if x][:4]
                with pytest.raises(IndexError):
                    loc[:keep + 1]
            del eng
    assert not bad, f"{name} {'half' if half else 'u8'}: {len(bad)} lines:\n" + "\n".join(bad[:25])


class ScanAndCorrectOnly:
    """A GpuShardEngine without sequential_scan: ShardedRender then runs its protocol — zero-state scan, carry, fix-up — on one rank too,
    instead of threading the state through the chunks."""

    def __init__(self, engine):
        self.engine, self.slots = engine, engine.slots

    def local_scan(self, frames, first_index, clip_start, slot=0):
        return self.engine.local_scan(frames, first_index, clip_start, slot=slot)

    def correct(self, local, carry, p, out):
        return self.engine.correct(local, carry, p, out)


@pytest.mark.parametrize("name,half", E2E, ids=E2E_IDS)
def test_protocol_against_model(env, name, half):
    """shard_model.sharded, exactly: ShardedRender's rounds on one rank (dist=None; the exact chain: the true final is carried) on the
    schedule whose chunks are shorter than the settling time, and the parallel hop (the chunk-final LOCAL state is the carry) run by hand
    on the two that are longer.  tests/test_shard_model.py bounds the model's distance to the in-order render on these very clips."""
    from pythoncrt_amd.shard import FrameShard, ShardedRender
    bad = []
    for h, w in sm.E2E_SHAPES:
        for p, chunk, keep in sm.SCHEDULES:
            cfg, point, eng = engine_for(name, half, h, w, p, chunk, keep)
            rule = sm.schedule_rule(p, chunk)
            frames = sm.clip(h, w, half, sm.E2E_CHUNKS * chunk)
            d_frames = up(np.stack(frames))
            m_out, m_carries = sm.sharded(frames, cfg, half, chunk, keep, rule, sm.E2E_FIRST, point)
            assert m_carries[0] is None and all(c is not None for c in m_carries[1:])
            parts = []
            if rule == "exact":
                render = ShardedRender(FrameShard(1, 0, chunk), p, ScanAndCorrectOnly(eng), dist=None)
                assert not render.parallel_hop and not render.overlap
                for r in range(sm.E2E_CHUNKS):
                    parts.append(render.run_round(d_frames[r * chunk:(r + 1) * chunk], r).cpu().numpy())
            else:
                assert ShardedRender(FrameShard(2, 0, chunk), p, eng, dist=None).parallel_hop
                carry = None
                for c in range(sm.E2E_CHUNKS):
                    loc, out = eng.local_scan(d_frames[c * chunk:(c + 1) * chunk], sm.E2E_FIRST + c * chunk, clip_start=(c == 0), slot=c % 2)
                    if carry is not None:
                        eng.correct(loc[:keep], carry, p, out[:keep])
                    carry = loc[chunk - 1].clone()          # what this rank sends on: its chunk-final local state
                    parts.append(out.cpu().numpy())
            got = np.concatenate(parts)
            lines = [describe(got[j], m_out[j], f"{h}x{w} p={p} chunk={chunk} ({rule}) frame {j}") for j in range(len(frames))]
            bad += [x for x in lines if x][:4]
            del eng
    assert not bad, f"{name} {'half' if half else 'u8'}: {len(bad)} lines:\n" + "\n".join(bad[:25])
