"""pythoncrt_amd — MI355X-native per-frame CRT effect chain behind PythonCRT's own API.

    from pythoncrt_amd import apply_crt_effect, apply_static_effects, make_triad_mask, make_vignette
    from pythoncrt_amd import process_frames      # the loop of process_video (ref:1037-1131) over the caller's frame iterator and writer
    from pythoncrt_amd import IngestResize        # its first step (ref:1039-1041) on the device: Pillow's BILINEAR resize of uint8 frames
    from pythoncrt_amd import EgressYuv           # its last step (ref:970-1002, `-pix_fmt yuv420p`) on the device: rgb24 -> yuv420p / nv12
    from pythoncrt_amd import UnpackYuv           # the step in front of it (the reader's `-pix_fmt rgb24`, ref:489-502) on the device: yuv420p / nv12 -> rgb24
    from pythoncrt_amd import UnpackYuv10, EgressYuv10   # the same two steps for a half chain: yuv420p10le / p010le <-> half RGB
    from pythoncrt_amd import UnpackYuv422, EgressYuv422 # the same two steps for 8-bit 4:2:2: yuv422p / yuyv422 / uyvy422 <-> rgb24
    from pythoncrt_amd import UnpackDeep444, EgressDeep444  # ... and for 10-bit 4:4:4 on a half chain: yuv444p10le / gbrp10le / x2rgb10le <-> half RGB
    from pythoncrt_amd import UnpackSited         # the source step of every 4:2:0 / 4:2:2 format with chroma interpolated at its siting ("left" / "center")
    from pythoncrt_amd import EgressSited         # ... and the egress step of the same formats with chroma filtered onto that siting instead of box-averaged
    from pythoncrt_amd import UnpackField420      # the source step of INTERLACED 4:2:0 material: every luma row takes chroma from rows of its own field
    from pythoncrt_amd import EgressField420      # ... and the egress step of an INTERLACED 4:2:0 delivery: every chroma sample formed from rows of its own field
    from pythoncrt_amd import ResizeHalf          # IngestResize for half frames: behind the chain, where process_frames(deliver_size=) delivers another size
    from pythoncrt_amd import Resample            # either of the two with a filter: box / bilinear / hamming / bicubic / lanczos, uint8 or half frames
    from pythoncrt_amd import Canvas              # crop and pad: a window of uint8 or half frames placed on a canvas of another size, the rest a colour
    from pythoncrt_amd import Widen, Narrow       # format=: uint8 frames to half exactly, half frames to uint8 rounded or with ordered dither
    from pythoncrt_amd import Deinterlace         # yadif's place: two fields woven into a frame become one progressive frame, or one per field
    from pythoncrt_amd import AdaptiveDeinterlace # ... motion-adaptive: the other field woven in where the picture stood still, "edge" where it moved
    from pythoncrt_amd import Interlace           # interlace / tinterlace's place: two finished frames woven into one 1080i / 576i / 480i frame, with a low-pass
    from pythoncrt_amd import Signal              # the cable: an NTSC-like composite / S-Video encode and decode of every row: bleed, dot crawl, rainbows
    from pythoncrt_amd import PalSignal           # ... and the PAL one: 270 degrees per line, the V switch, a delay-line decoder with a phase error
    from pythoncrt_amd import probe_frames        # cropdetect / idet / signalstats' place: letterbox, field order and levels measured on the device,
    from pythoncrt_amd import Probe, ProbeReport  # ... as keywords for process_frames; the plan that writes the records, the report that reads them
    from pythoncrt_amd import Lut3D, Cube         # lut3d=: a .cube colour LUT applied with tetrahedral interpolation, uint8 or half frames

See DESIGN.md (path, kernels, roofline) and INTEGRATION.md (how the reference binds to it).
"""
from .effects import (DeviceState, TriadMask, VignetteMask, apply_crt_effect, apply_static_effects, make_triad_mask,
                      make_vignette)
from .canvas import Canvas
from .deep import EgressYuv10, UnpackYuv10
from .depth import Narrow, Widen
from .adeint import AdaptiveDeinterlace
from .deint import Deinterlace
from .deep444 import EgressDeep444, UnpackDeep444
from .egress import EgressYuv
from .field420 import EgressField420, UnpackField420
from .ingest import IngestResize
from .interlace import Interlace
from .cube import Cube
from .lut3d import Lut3D
from .pal import PalSignal
from .resize16 import ResizeHalf
from .resample import Resample
from .render import iter_deep444, iter_rgb24, iter_yuv420, iter_yuv422, process_frames
from .signal import Signal
from .sited import EgressSited, UnpackSited
from .unpack import UnpackYuv
from .yuv422 import EgressYuv422, UnpackYuv422

__all__ = ["DeviceState", "TriadMask", "VignetteMask", "apply_crt_effect", "apply_static_effects", "make_triad_mask", "make_vignette",
           "process_frames", "iter_rgb24", "iter_yuv420", "IngestResize", "EgressYuv", "UnpackYuv", "EgressYuv10", "UnpackYuv10",
           "iter_yuv422", "EgressYuv422", "UnpackYuv422", "iter_deep444", "EgressDeep444", "UnpackDeep444", "UnpackSited", "EgressSited", "UnpackField420", "EgressField420", "ResizeHalf", "Resample", "Canvas", "Widen", "Narrow", "Deinterlace", "AdaptiveDeinterlace", "Lut3D", "Cube", "Interlace", "Signal", "PalSignal", "Probe", "ProbeReport", "probe_frames"]


def __getattr__(name):
    """The probe's names on first use: `python -m pythoncrt_amd.probe` then finds its module not yet imported by the package."""
    if name in ("Probe", "ProbeReport", "probe_frames"):
        from . import probe
        return getattr(probe, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
