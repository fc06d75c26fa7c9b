"""The sweep of the whole chain on the GPU: every case of tests/chain_model.py — 48 seeded draws of admitted options and the explicit
cases, up to 14 stages around the chain at once — runs through the two ends alone (every intermediate buffer compared, the first
diverging stage named), through process_frames (the effect chain a FramePipeline run by the test in the render loop's batches) and, for
eight draws, through the CLI; three explicit rgb24 streams change their source size up to twelve times, past the four source ends the
render loop keeps.  Exact: half frames are compared as bits, everything else with array_equal; there is no tolerance."""
import functools

import numpy as np
import pytest

from pythoncrt_amd import formats, options
from tests import chain_model as cm
from tests import lut3d_model
from tests.deint_model import bits

pytestmark = pytest.mark.gpu

SEED = 29
CASES = cm.cases()
BY_ID = {c["id"]: c for c in CASES + list(cm.STREAMS)}


def _id(case):
    return case["id"]


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _pipe(frames, lengths):
    """A FramePipeline of the frames' dtype with process_frames' default settings over [n, h, w, 3], in batches of `lengths` frames with the
    frame index running on and the state carried as the render loop carries it."""
    import torch
    from pythoncrt_amd.pipeline import FramePipeline, RenderSettings
    h, w = frames.shape[1:3]
    x = torch.from_numpy(np.ascontiguousarray(frames)).to(_dev())
    pipe = FramePipeline(_dev(), h, w, RenderSettings(), fps=30.0, noise_seed=SEED, dtype=x.dtype)
    outs, state, lo = [], None, 0
    for m in lengths:
        out, state = pipe.run(x[lo:lo + m], first_index=lo, state=state)
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
        lo += m
    assert lo == x.shape[0]
    return np.concatenate(outs)


def _render(case):
    """What process_frames hands its writer for the case, and what its loop asked of the source ends: (frames, the return value, the log of
    ("restart", size) and ("convert", size, slot, source frames, the index the Signal is given, frames written))."""
    import pythoncrt_amd as pc
    from pythoncrt_amd import ends
    got, log = [], []
    convert, restart = ends.SourceEnd.convert, ends.SourceEnd.restart

    def logged_convert(self, d, n, dst):
        log.append(("convert", self.src_hw, d, n, self.index, int(dst.shape[0])))
        return convert(self, d, n, dst)

    def logged_restart(self):
        log.append(("restart", self.src_hw))
        return restart(self)
    ends.SourceEnd.convert, ends.SourceEnd.restart = logged_convert, logged_restart
    try:
        h, w = case["render"]
        wrote = pc.process_frames(iter(cm.frames(case)), lambda a: got.append(np.array(a)), w, h, 30.0, cm.delivered_count(case), noise_seed=SEED,
                                  batch=case["batch"], **cm.keywords(case))
    finally:
        ends.SourceEnd.convert, ends.SourceEnd.restart = convert, restart
    return got, wrote, log


def _loop(case):
    """The log the render loop must leave: batches alternate between the two slots, a batch is cut where the source size changes, a source
    end is told to restart where its batch does not continue the one before, and the Signal is given the stream index of the batch's first
    SOURCE frame — 0 where there is no Signal."""
    d, log, last = cm.Derived(case), [], None
    for k, (lo, n, hw) in enumerate(cm.batches(case)):
        key = hw if cm.source_stages(case, hw) else None                      # None: uploaded straight into the chain's input
        if key is not None:
            log += [("restart", hw)] * (key != last) + [("convert", hw, k % 2, n, lo if case["kw"]["in_signal"] != "rgb" else 0, n * d.ratio)]
        last = key
    return log


def _loop_held(case, log):
    exp = _loop(case)
    bad = next((i for i, (a, b) in enumerate(zip(log, exp)) if a != b), None if len(log) == len(exp) else min(len(log), len(exp)))
    assert bad is None, (case["id"], "the render loop diverges at call", bad, "(kind, size, slot, source frames, Signal index, frames written): got",
                         log[bad:bad + 1], "the batches state", exp[bad:bad + 1])


@functools.lru_cache(maxsize=None)
def _rendered(case_id):
    """_render of a case, once for the tests that share it."""
    return _render(BY_ID[case_id])


def _differs(got, exp):
    """None where the device buffer holds the model's frames, else (the first frame that differs, samples that differ) or the two shapes."""
    g, e = got.cpu().numpy(), np.asarray(exp)
    if g.shape != e.shape or g.dtype != e.dtype:
        return (g.shape, str(g.dtype), e.shape, str(e.dtype))
    g, e = bits(g), bits(e)
    return next(((i, int((g[i] != e[i]).sum())) for i in range(len(g)) if not np.array_equal(g[i], e[i])), None)


def _held(case, got, exp):
    """The written frames are the models': count, the size of every frame, every byte."""
    assert len(got) == len(exp) == cm.delivered_count(case), (case["id"], len(got), len(exp))
    size, fmt = cm.delivery_geometry(case)[4], case["kw"]["out_pix_fmt"]
    shape = size + (3,) if fmt == "rgb24" else (formats.frame_bytes(size[0], size[1], fmt),)
    per = []
    d = cm.Derived(case)
    for b, (_, n, _) in enumerate(cm.batches(case)):
        per += [b] * d.delivered(n * d.ratio)
    for i, (g, e) in enumerate(zip(got, exp)):
        assert g.shape == shape == e.shape and g.dtype == np.uint8, (case["id"], i, g.shape, shape)
        assert np.array_equal(g, e), (case["id"], "delivered frame", i, "of batch", per[i], "samples that differ", int((g != e).sum()))
    assert not np.array_equal(got[0], got[-1])                                # frames of a render, not one constant


@pytest.mark.parametrize("case", CASES + list(cm.STREAMS), ids=_id)
def test_ends_alone(case):
    """The source ends and the delivery end as the render loop drives them — two slots, the batch's first stream index, restart() at a
    change of size — with a device copy in the chain's place: every buffer behind every stage holds the composer's frames."""
    import torch
    dev, d = _dev(), cm.Derived(case)
    spec = options.ChainOptions.build(cm.raw(case), "keywords")
    pix = torch.float16 if spec.half else torch.uint8
    h, w = case["render"]
    items = cm.frames(case)
    exp, trace = cm.expect(case, source=cm.cached_source(case))
    end = spec.delivery_end(dev, pix)
    dev_in = [torch.empty((d.B, h, w, 3), dtype=pix, device=dev) for _ in range(2)]
    dev_out = [torch.empty((d.B, h, w, 3), dtype=pix, device=dev) for _ in range(2)]
    end.slots(dev_out)
    sources, last, sent_all = {}, None, []
    for k, ((lo, n, hw), tr) in enumerate(zip(cm.batches(case), trace)):
        slot, m, got = k % 2, n * d.ratio, []
        if tr[0][0] == "upload":                                              # an rgb24 frame at render size, straight into the chain's input
            dev_in[slot][:n].copy_(torch.from_numpy(np.stack(items[lo:lo + n])).to(dev))
        else:
            src = sources.get(hw)
            if src is None:
                src = sources[hw] = spec.source_end(dev, hw, pix).slots(d.Bs, 2, pinned=False)
            if hw != last:
                src.restart()
            src.index = lo
            staged = np.stack([np.asarray(a).reshape(src.frame_shape) for a in items[lo:lo + n]])
            src.dev[slot][:n].copy_(torch.from_numpy(staged).to(dev))
            src.convert(slot, n, dev_in[slot][:m])
            got += [src.mid[i][slot][:len(tr[i][3])] for i in range(len(src.stages) - 1)]
        last = hw
        got.append(dev_in[slot][:m])
        dev_out[slot][:m].copy_(dev_in[slot][:m])                             # the "chain"
        got.append(dev_out[slot][:m])
        sent = end.run(slot, m)
        base = len(got)
        got += [end.bufs[i][slot][:len(tr[base + i][3])] for i in range(len(end.stages))]
        if end.egress is not None:
            got.append(sent)
        torch.cuda.synchronize()
        assert len(got) == len(tr), (case["id"], k, len(got), [s[0] for s in tr])
        assert sent.data_ptr() == got[-1].data_ptr() and len(sent) == d.delivered(m)
        for buf, (name, size, dt, frames) in zip(got, tr):
            bad = _differs(buf, frames)
            assert bad is None, (case["id"], "the first stage that diverges", name, size, dt, "batch", k, "slot", slot, "frame, samples" if len(bad) == 2 else "shapes", bad)
        sent_all += list(sent.cpu().numpy())
    _held(case, sent_all, exp)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_process_frames(case):
    got, wrote, log = _rendered(case["id"])
    _loop_held(case, log)
    exp, _ = cm.expect(case, _pipe, source=cm.cached_source(case))
    assert wrote == len(got)
    _held(case, got, exp)


@pytest.mark.parametrize("case", cm.STREAMS, ids=_id)
def test_streams_of_many_source_sizes(case, monkeypatch):
    """rgb24, batch 2, persistence at its default.  Six sizes in the order A A B B C C D D E E A A F: A's source end is dropped when E
    arrives (the table keeps four) and built again — seven ends for six sizes —, the Signal's index counts on, the adaptive history
    restarts at every change, and the new end of A gives a fresh one's bytes: what `expect` states."""
    built = []
    source_end = options.ChainOptions.source_end

    def logged(self, device, src_hw, pix):
        built.append(tuple(src_hw))
        return source_end(self, device, src_hw, pix)
    monkeypatch.setattr(options.ChainOptions, "source_end", logged)
    got, wrote, log = _render(case)
    _loop_held(case, log)
    runs = [s for i, s in enumerate(case["sizes"]) if i == 0 or s != case["sizes"][i - 1]]
    if len(set(case["sizes"])) == 6:
        assert runs == [cm._A, cm._B, cm._C, cm._D, cm._E, cm._A, cm._F] and built == runs      # A twice: evicted, then built again
    else:
        assert built == sorted(set(runs), key=runs.index)                      # at most four sizes: every end is built once and kept
    exp, _ = cm.expect(case, _pipe, source=cm.cached_source(case))
    assert wrote == len(got)
    _held(case, got, exp)


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------------------

CLI_CASES = [c for c in cm.draws() if set(c["sizes"]) == {c["render"]}][:8]       # the CLI reads frames of the render size


def _flags(case, tmp_path):
    kw, (h, w) = case["kw"], case["render"]
    f = ["--width", str(w), "--height", str(h), "--fps", "30", "--batch", str(case["batch"]), "--noise-seed", str(SEED)]
    for key in ("in_pix_fmt", "out_pix_fmt", "in_matrix", "in_range", "out_matrix", "out_range", "in_chroma", "in_chroma_rows", "out_chroma", "in_filter",
                "deinterlace", "field_order", "deinterlace_fields", "in_signal", "signal_chroma", "chain_pix", "dither", "deliver_filter", "deliver_fit",
                "deliver_interlace", "deliver_lowpass"):
        f += ["--" + key.replace("_", "-"), str(kw[key])]
    f += ["--signal-crawl", "on" if kw["signal_crawl"] else "off", "--deliver-pad-color", ",".join(map(str, kw["deliver_pad_color"]))]
    if kw["in_crop"] is not None:
        y, x, ch, cw = kw["in_crop"]
        f += ["--in-crop-y", str(y), "--in-crop-x", str(x), "--in-crop-height", str(ch), "--in-crop-width", str(cw)]
    if kw["deliver_size"] is not None:
        f += ["--deliver-height", str(kw["deliver_size"][0]), "--deliver-width", str(kw["deliver_size"][1])]
    for flag, key in (("--in-lut", "in_cube"), ("--deliver-lut", "deliver_cube")):
        if case[key] is not None:
            path = tmp_path / (key + ".cube")
            lut3d_model.write_cube(path, cm.cube(case[key]).values)
            f += [flag, str(path)]
    return f


def test_the_cli_cases_are_eight():
    assert len(CLI_CASES) == 8


@pytest.mark.parametrize("k", range(8))
def test_cli_writes_the_same_bytes(tmp_path, k):
    """The case written as flags, file to file: the output file holds the bytes process_frames handed its writer."""
    from pythoncrt_amd import cli
    case, io = CLI_CASES[k], ("staged", "mapped")[k % 2]
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    src.write_bytes(b"".join(np.ascontiguousarray(a).tobytes() for a in cm.frames(case)))
    assert cli.main(["--input", str(src), "--output", str(dst), "--io", io] + _flags(case, tmp_path)) == 0
    got = _rendered(case["id"])[0]
    written = np.frombuffer(dst.read_bytes(), dtype=np.uint8)
    fb = got[0].size
    assert written.size == len(got) * fb, (case["id"], io, written.size, len(got), fb)
    for i, g in enumerate(got):
        assert np.array_equal(written[i * fb:(i + 1) * fb], g.reshape(-1)), (case["id"], io, i)
