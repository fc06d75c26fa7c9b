"""pythoncrt_amd.cli against the reference's own CLI (tests/golden/reference_cli.json, made by
gen_golden.py from parse_args ref:1153-1207 and main ref:1210-1267): same flag names and
defaults, same clamps on the way to the render settings."""
import json
import os

import numpy as np

from pythoncrt_amd import cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_cli.json")))
ARGVS = {
    "defaults": ["--input", "x.mp4"],
    "extremes_hi": ["--input", "x.mp4", "--scanline-strength", "5", "--triad-strength", "3", "--triad-gamma", "0.01", "--triad-softness", "-1",
                    "--aberration-px", "40", "--bloom-sigma", "-2", "--bloom-strength", "-1", "--noise-strength", "-3", "--vignette-strength", "9",
                    "--persistence", "0.99", "--scanline-period", "0.2", "--pixel-size", "0", "--gamma", "0", "--saturation", "-1",
                    "--temperature", "4", "--flicker-strength", "7", "--flicker-hz", "-1", "--grain-size", "0", "--scanline-thickness", "0.01",
                    "--warp-strength", "3", "--glitch-amp", "-5", "--glitch-height", "2", "--bloom-threshold", "1.5", "--crf", "99"],
    "extremes_lo": ["--input", "x.mp4", "--scanline-strength", "-1", "--aberration-px", "-40", "--persistence", "-0.5", "--temperature", "-4",
                    "--warp-strength", "-3", "--vignette-strength", "-1", "--bloom-threshold", "-1", "--crf", "1", "--no-fast-bloom",
                    "--triad-preserve-luma", "--text-after", "--fps", "25", "--width", "640", "--height", "360"],
}
# process_video keyword -> RenderSettings field
RENAME = {"target_bitrate_kbps": None, "input_path": None, "output_path": None, "width": None, "height": None, "fps": None, "crf": None,
          "gpu": None, "nvenc_preset": None, "encoder_preference": None, "decoder_preference": None, "text": None, "text_font": None,
          "text_size": None, "text_color": None, "text_pos": None, "text_after": None}


def test_flag_names_and_defaults():
    ours = vars(cli.build_parser().parse_args([]))
    ref = FX["namespace_defaults"]
    for k, v in ref.items():
        assert k in ours, k
        assert ours[k] == v, (k, ours[k], v)
    assert set(ours) - set(ref) == {"batch", "noise_seed", "staging_report", "io"}      # the additions documented in cli.py


def test_clamps_match_reference_main():
    for name, argv in ARGVS.items():
        rs = cli.settings_from_args(cli.build_parser().parse_args(argv))
        ref = FX["process_video_kwargs"][name]
        for k, v in ref.items():
            if k in RENAME:
                continue
            assert getattr(rs, k) == v, (name, k, getattr(rs, k), v)


def test_process_frames_takes_process_video_keywords():
    """pythoncrt_amd.process_frames — the drop-in for the loop of process_video (ref:1037-1131) — accepts every keyword process_video itself
    takes (tests/golden/reference_cli.json holds the reference's own parameter list): the effect keywords by name with the CLI's defaults, the
    container / codec ones (input_path, crf, nvenc_preset, ...) swallowed, anything else refused; its leading parameters are the things the
    reference's loop already holds (frame iterator, writer call, output size, fps, total_frames)."""
    import inspect
    import pythoncrt_amd as pc
    from pythoncrt_amd import render
    sig = inspect.signature(pc.process_frames)
    names = list(sig.parameters)
    assert names[:6] == ["frame_iter", "write_frame", "out_w", "out_h", "fps_out", "total_frames"]
    ref = FX["process_video_kwargs"]["defaults"]
    io_keys = set(render._IO_KEYS)
    for k, v in ref.items():
        if k in io_keys:
            assert k not in sig.parameters
            continue
        p = sig.parameters[k]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY, k
        if k == "text_pos":
            assert tuple(p.default) == tuple(v)
        elif k == "text_after":
            assert p.default is True                          # process_video's own default (ref:910); the CLI passes its flag, off by default (ref:1199)
        elif k != "progress_cb":
            assert p.default == v, (k, p.default, v)          # = what process_video receives when the CLI is run with no flags
    assert set(ref) - io_keys <= set(names)
    assert sig.parameters["io_keywords"].kind is inspect.Parameter.VAR_KEYWORD


def test_process_frames_fails_loudly_without_a_gpu():
    """No CPU fallback in the product path: without a ROCm device process_frames raises (and a misspelt keyword is refused before anything else)."""
    import pytest
    import torch
    import pythoncrt_amd as pc
    with pytest.raises(TypeError):
        pc.process_frames(iter([]), lambda a: None, 8, 8, 30, 1, scanlines=1.0)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no ROCm device"):
            pc.process_frames(iter([np.zeros((8, 8, 3), np.uint8)]), lambda a: None, 8, 8, 30, 1)


def test_iter_rgb24_is_the_raw_readers_iteration():
    """pythoncrt_amd.iter_rgb24 = FFmpegRawReader.iter_frames (ref:495-506) over an open stream: whole frames in order, a trailing partial frame
    dropped, short reads of a pipe reassembled."""
    import io
    import pythoncrt_amd as pc
    h, w, n = 5, 7, 4
    data = np.arange(n * h * w * 3, dtype=np.uint32).astype(np.uint8).tobytes()
    got = list(pc.iter_rgb24(io.BytesIO(data + b"\x01\x02\x03"), w, h))
    assert len(got) == n and all(g.shape == (h, w, 3) and g.dtype == np.uint8 for g in got)
    assert b"".join(g.tobytes() for g in got) == data

    class Dribble:                                      # a pipe that hands out at most 11 bytes per read
        def __init__(self, b):
            self.b, self.p = b, 0

        def read(self, k):
            out = self.b[self.p:self.p + min(k, 11)]
            self.p += len(out)
            return out
    got2 = list(pc.iter_rgb24(Dribble(data), w, h))
    assert len(got2) == n and b"".join(g.tobytes() for g in got2) == data
    assert list(pc.iter_rgb24(io.BytesIO(b""), w, h)) == []
