"""probe_frames, the report and the command-line module on the GPU: synthetic letterboxed TFF / BFF / progressive streams
(tests/probe_model.py) as rgb24, nv12, uyvy422 and p010le, probed in batches smaller than the stream.  The window and the field order are
recovered, the records are the model's on the RGB the source plan writes, and process_frames(**report.suggest()) renders the picture area."""
import json

import numpy as np
import pytest

from pythoncrt_amd import cli, formats, probe
from tests import probe_model as model

pytestmark = pytest.mark.gpu

PIC, FULL, AT = (160, 32), (176, 48), (8, 8)        # a tall picture: the still edges above and below it comb too, and must stay small beside it
FMTS = ("rgb24", "nv12", "uyvy422", "p010le")
KINDS = ("tff", "bff", "progressive")
MARGIN = 1.5
N = 6


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


_streams = {}


def stream(fmt, kind):
    """(the items of the frame iterator, the RGB frames the source plan writes as a numpy array): the boxed scene, packed as `fmt` by the
    project's own egress plan.  Built once per (fmt, kind)."""
    import torch
    if (fmt, kind) not in _streams:
        rgb = model.boxed(model.scene(kind, N, PIC[0], PIC[1]), FULL, AT)
        if fmt == "rgb24":
            _streams[fmt, kind] = (list(rgb), rgb)
        else:
            deep = formats.bits(fmt) == 10
            x = torch.from_numpy(rgb).to(_dev())
            packed = formats.egress_plan(_dev(), FULL, fmt, "bt601", "tv", "center").run(x.to(torch.float16) if deep else x)
            back = formats.source_plan(_dev(), FULL, fmt, "bt601", "tv", "replicate").run(packed)
            torch.cuda.synchronize()
            _streams[fmt, kind] = (list(packed.cpu().numpy()), back.cpu().numpy())
    return _streams[fmt, kind]


def _same_report(got, exp):
    for name in ("frames", "pairs", "s_cur", "s_even", "s_odd", "sum_y", "rgb_min", "rgb_max"):
        assert getattr(got, name) == getattr(exp, name), name
    for name in ("hist", "row_max", "col_max"):
        assert np.array_equal(getattr(got, name), getattr(exp, name)), name


@pytest.mark.parametrize("fmt", FMTS)
def test_probe_frames_recovers_the_window_and_the_order(fmt):
    import pythoncrt_amd as pc
    packed = {} if fmt == "rgb24" else dict(in_pix_fmt=fmt, in_size=FULL)
    for kind in KINDS:
        items, rgb = stream(fmt, kind)
        rep = pc.probe_frames(iter(items), FULL[1], FULL[0], batch=4, **packed)            # 4 + 2 frames
        exp = probe.ProbeReport(FULL).add(model.records(rgb))                               # the model on the RGB the source plan writes
        _same_report(rep, exp)
        e, o = exp.s_even, exp.s_odd
        if kind == "progressive":
            assert MARGIN * max(e, o) <= probe.RATIO * min(e, o), (fmt, kind, e, o)
        else:
            big, small = (e, o) if kind == "tff" else (o, e)
            assert big >= MARGIN * probe.RATIO * small, (fmt, kind, e, o)                   # the scene keeps its margin behind the format's round trip
        assert rep.field_order() == kind and rep.crop() == AT + PIC and rep.frames == N and rep.pairs == N - 1
        want = {"in_crop": AT + PIC} if kind == "progressive" else {"in_crop": AT + PIC, "deinterlace": "adaptive", "field_order": kind}
        assert rep.suggest() == want
        lv = rep.levels()
        assert lv["luma_min"] <= 8 and lv["luma_max"] >= 100 and 0 < lv["luma_mean"] < 255
        # one batch, and a stream cut short: the same report whatever the batches; max_frames counts frames
        _same_report(pc.probe_frames(iter(items), FULL[1], FULL[0], batch=16, **packed), exp)
        short = pc.probe_frames(iter(items), FULL[1], FULL[0], batch=2, max_frames=3, **packed)
        _same_report(short, probe.ProbeReport(FULL).add(model.records(rgb[:3])))
    # ... and the render the report asks for delivers the picture area
    kind = KINDS[FMTS.index(fmt) % len(KINDS)]
    items, _ = stream(fmt, kind)
    rep = pc.probe_frames(iter(items), FULL[1], FULL[0], batch=4, **packed)
    got = []
    extra = dict(chain_pix="half") if fmt == "p010le" else {}
    n = pc.process_frames(iter(items), lambda a: got.append(np.array(a)), PIC[1], PIC[0], 30.0, N, batch=4, noise_seed=1, **packed, **extra, **rep.suggest())
    assert n == N == len(got) and all(a.shape == PIC + (3,) and a.dtype == np.uint8 for a in got)
    assert min(int(a.mean()) for a in got) > 8                                               # the picture, not the bars


def test_rgb24_frames_of_two_sizes_and_an_empty_stream():
    import pythoncrt_amd as pc
    items, _ = stream("rgb24", "tff")
    with pytest.raises(ValueError, match="more than one size"):
        pc.probe_frames(iter(items[:2] + [items[2][:, :40]]), FULL[1], FULL[0])
    with pytest.raises(ValueError, match="H x W x 3"):
        pc.probe_frames(iter([items[0][..., 0]]), FULL[1], FULL[0])
    with pytest.raises(ValueError, match="holds"):
        pc.probe_frames(iter([np.zeros(7, dtype=np.uint8)]), FULL[1], FULL[0], in_pix_fmt="nv12")
    empty = pc.probe_frames(iter(()), FULL[1], FULL[0], in_pix_fmt="nv12")
    assert empty.frames == 0 and empty.size == FULL and empty.suggest() == {} and empty.levels() == {} and empty.field_order() is None


@pytest.mark.parametrize("fmt", ["rgb24", "uyvy422"])
def test_the_command_line_module_on_a_file(fmt, tmp_path, capsys):
    items, rgb = stream(fmt, "bff")
    src = tmp_path / f"in.{fmt}"
    src.write_bytes(b"".join(np.ascontiguousarray(a).tobytes() for a in items))
    base = ["--input", str(src), "--width", str(FULL[1]), "--height", str(FULL[0]), "--in-pix-fmt", fmt]
    assert probe.main(base) == 0
    line = capsys.readouterr().out.strip()
    exp = probe.ProbeReport(FULL).add(model.records(rgb))
    assert line.split() == exp.flags() and "--field-order bff" in line
    a = cli.add_input_flags(cli.add_output_flags(cli.build_parser())).parse_args(
        ["--input", str(src), "--output", str(tmp_path / "out.rgb"), "--width", str(FULL[1]), "--height", str(FULL[0]), "--in-pix-fmt", fmt] + line.split())
    spec, ranks = cli.check_flags(a)                                                        # the line parses with cli's own parser and passes its rules
    assert spec.crop == AT + PIC and spec.deinterlace == ("adaptive", "bff", "first") and ranks is None
    assert probe.main(base + ["--json", "--frames", "4"]) == 0
    got = json.loads(capsys.readouterr().out)
    want = probe.ProbeReport(FULL).add(model.records(rgb[:4])).as_dict()
    assert got == json.loads(json.dumps(want)) and got["frames"] == 4 and got["field_order"] == "bff" and got["crop"] == list(AT + PIC)
    assert json.loads(json.dumps(got)) == got
