"""Command line of the reference (crt_filter.py parse_args ref:1153-1207, clamps in main
ref:1220-1267) over the GPU pipeline.

Same flag names, defaults and clamps: `build_parser` restates the flag schema of `parse_args` (ref:1154-1206) and `settings_from_args` the
clamp list of `main()` (ref:1225-1266) — the drop-in contract IS those names, defaults and bounds, so these two blocks follow
crt_filter.py (PythonCRT, GPL-3.0) line for line and are pinned against it by tests/golden/reference_cli.json.  What differs is the container I/O, which is out of scope
here (codec plumbing): frames are read and written as raw `rgb24` (H x W x 3 uint8,
the wire format of the reference's own FFmpegRawReader, ref:489-502, and of its ffmpeg writer
pipe), from a file or stdin/stdout, so the drop-in sits between two ffmpeg processes:

    ffmpeg -i in.mp4 -f rawvideo -pix_fmt rgb24 - |
      python -m pythoncrt_amd.cli --input - --width 1920 --height 1080 --fps 30 --output - [effect flags] |
      ffmpeg -f rawvideo -pix_fmt rgb24 -s 1920x1080 -r 30 -i - out.mp4

With `--out-pix-fmt yuv420p` (or `nv12`; `--out-matrix bt601|bt709`, `--out-range tv|pc`) the finished frames are converted to the
encoder's 4:2:0 format on the GPU (include/crtfx_egress.h) and leave as 1.5 bytes per pixel instead of 3 — half the download, half the
pipe, and no conversion left for the encoder:

      python -m pythoncrt_amd.cli --input - --width 1920 --height 1080 --fps 30 --output - --out-pix-fmt yuv420p [effect flags] |
      ffmpeg -f rawvideo -pix_fmt yuv420p -s 1920x1080 -r 30 -i - out.mp4

With `--in-pix-fmt yuv420p` (or `nv12`; `--in-matrix bt601|bt709`, `--in-range tv|pc`) the source frames are read in the decoder's 4:2:0
format and converted to RGB on the GPU (include/crtfx_unpack.h): 1.5 bytes per pixel through the pipe, the pinned slot and PCIe instead of
3, and no `-pix_fmt rgb24` conversion in front.  Both ends together — no host core touches a pixel:

    ffmpeg -i in.mp4 -f rawvideo -pix_fmt nv12 - |
      python -m pythoncrt_amd.cli --input - --width 1920 --height 1080 --fps 30 --output - --in-pix-fmt nv12 --out-pix-fmt nv12 [effect flags] |
      ffmpeg -f rawvideo -pix_fmt nv12 -s 1920x1080 -r 30 -i - out.mp4

With `yuv420p10le` or `p010le` on BOTH ends a 10-bit stream goes decoder -> chain -> encoder at 3 bytes per pixel each way and the chain runs
on half pixels (include/crtfx_deep.h); one end only is refused:

    ffmpeg -i in10.mkv -f rawvideo -pix_fmt p010le - |
      python -m pythoncrt_amd.cli --input - --width 3840 --height 2160 --fps 30 --output - --in-pix-fmt p010le --out-pix-fmt yuv420p10le [effect flags] |
      ffmpeg -f rawvideo -pix_fmt yuv420p10le -s 3840x2160 -r 30 -i - out.mkv

`yuv444p10le`, `gbrp10le` and `x2rgb10le` (10-bit 4:4:4: ProRes 4444 / DNxHR 444 decodes, DPX / TIFF / EXR sequences, screen capture) are
members of that 10-bit family, in any pairing with it (include/crtfx_444.h): 6 bytes per pixel, 4 for x2rgb10le, no chroma sample dropped
on either end; `--in-matrix` / `--in-range` / `--out-matrix` / `--out-range` apply to yuv444p10le, the two RGB formats are full range and
ignore them:

    ffmpeg -i prores4444.mov -f rawvideo -pix_fmt yuv444p10le - |
      python -m pythoncrt_amd.cli --input - --width 1920 --height 1080 --fps 24 --output - --in-pix-fmt yuv444p10le --out-pix-fmt gbrp10le [effect flags] |
      ffmpeg -f rawvideo -pix_fmt gbrp10le -s 1920x1080 -r 24 -i - out_%06d.dpx

`yuv422p`, `yuyv422` and `uyvy422` (8-bit 4:2:2: capture cards, mezzanine codecs) are taken and written like the 8-bit 4:2:0 formats, on
either end independently of the other (include/crtfx_422.h): 2 bytes per pixel, and the source's vertical chroma is kept on the way out:

    ffmpeg -f v4l2 -i /dev/video0 -f rawvideo -pix_fmt uyvy422 - |
      python -m pythoncrt_amd.cli --input - --width 1920 --height 1080 --fps 30 --output - --in-pix-fmt uyvy422 --out-pix-fmt yuv422p [effect flags] |
      ffmpeg -f rawvideo -pix_fmt yuv422p -s 1920x1080 -r 30 -i - out.mov

With a 4:2:0 / 4:2:2 `--in-pix-fmt`, `--in-chroma left` (MPEG-2 / H.264 / HEVC sources: ffprobe's chroma_location=left, or nothing) or
`--in-chroma center` (JPEG-family sources) interpolates chroma at its siting on the GPU instead of replicating each sample over its pixels
(UnpackSited, include/crtfx_sited.h); the default `replicate` is the path as it was.

With a 4:2:0 `--in-pix-fmt` from an interlaced encoder (DVD, 480i / 576i / 1080i broadcast), `--in-chroma-rows interlaced` takes chroma rows
0, 2, 4, ... as the top field's and 1, 3, 5, ... as the bottom field's, so that every luma row gets the colour of its own field
(UnpackField420, include/crtfx_field420.h) and `--deinterlace` reads fields whose colour is their own; the default `progressive` is the
path as it was.

With a 4:2:0 / 4:2:2 `--out-pix-fmt`, `--out-chroma left` filters every chroma sample onto its first luma column on the GPU
(EgressSited, include/crtfx_egress_sited.h) — the siting ffmpeg's muxers tag or assume for such a file, what ffprobe then reports as
chroma_location=left (or nothing) and the only siting 4:2:2 defines; pass `-chroma_sample_location left` to the encoder.  The default
`center` writes the 2 x 2 / 2 x 1 box mean as before (ffprobe's chroma_location=center: JPEG / MPEG-1).

`--in-crop-x / -y / -width / -height` cut a window out of every input frame on the GPU (include/crtfx_canvas.h) and resize it back to
`--width x --height` (a letterboxed source: the picture area fills the tube); with `--deliver-width` / `--deliver-height`, `--deliver-fit pad`
centres the render, resized to fit, on a frame of `--deliver-pad-color` (a 4:3 render pillarboxed in 16:9) and `--deliver-fit crop` cuts the
centred window of the delivery's aspect; the default `stretch` is the path as it was.

`--chain-pix half` runs the chain on half pixels whatever the formats (include/crtfx_depth.h), so the two ends need not have the same
depth — a 10-bit master delivered as 8-bit 4:2:0, no host `format=` filter around the tool:

    ffmpeg -i prores.mov -f rawvideo -pix_fmt p010le - |
      python -m pythoncrt_amd.cli --input - --width 1920 --height 1080 --fps 24 --output - --in-pix-fmt p010le --out-pix-fmt yuv420p \
             --chain-pix half --dither ordered [effect flags] |
      ffmpeg -f rawvideo -pix_fmt yuv420p -s 1920x1080 -r 24 -i - out.mp4

An 8-bit source is widened to half behind its own uint8 stages, an 8-bit delivery is narrowed at the delivery size behind the half
geometry, and `--dither ordered` adds an 8 x 8 Bayer threshold there instead of rounding to nearest (`none`, the default).  The default
`--chain-pix auto` is the path as it was, the one-end refusal included; `--dither ordered` needs `--chain-pix half` and an 8-bit output.

`--deinterlace linear|edge` takes every input frame as two woven fields and deinterlaces it on the GPU before anything else sees it
(include/crtfx_deint.h), `--field-order tff|bff` says which field comes first, and `--deinterlace-fields both` writes one frame per FIELD:
the chain then runs at field rate and `--persistence` decays field to field, as phosphor does.  Pass the field rate as `--fps`; the output
holds twice the input's frames.  `--deinterlace adaptive` is motion-adaptive (include/crtfx_adeint.h): where the picture did not change
since the previous input frame the missing rows are the other field's own (HUDs, text and backgrounds keep their full vertical resolution
and do not bob), where it changed they are `edge`'s; it looks one frame back only, so it adds no latency.
A 480i uyvy422 capture sent as fields, no host `yadif` in front of the tool:

    ffmpeg -i capture_480i.avi -f rawvideo -pix_fmt uyvy422 - |
      python -m pythoncrt_amd.cli --input - --width 720 --height 480 --fps 60 --output - --in-pix-fmt uyvy422 \
             --deinterlace edge --field-order bff --deinterlace-fields both [effect flags] |
      ffmpeg -f rawvideo -pix_fmt rgb24 -s 720x480 -r 60000/1001 -i - out.mp4

`--deliver-interlace tff|bff` delivers interlaced frames: every two consecutive finished frames are woven into one on the GPU
(include/crtfx_interlace.h), behind the delivery resize and the pad and in front of the dither and the output format, the first frame of
a pair giving the even rows (tff) or the odd rows (bff); `--deliver-lowpass linear|complex` filters every row vertically inside its own
frame first, against line twitter.  With `--deinterlace-fields both` in front, a 29.97i tape runs through the chain at field rate and
leaves as 29.97i, without a second ffmpeg process for `interlace` / `tinterlace`; the output holds half the chain's frames (an odd last
one is woven with itself).  480i in, 480i out, for a DVD encoder:

    ffmpeg -i capture_480i.avi -f rawvideo -pix_fmt uyvy422 - |
      python -m pythoncrt_amd.cli --input - --width 720 --height 480 --fps 60 --output - --in-pix-fmt uyvy422 --out-pix-fmt uyvy422 \
             --deinterlace edge --field-order bff --deinterlace-fields both --deliver-interlace bff --deliver-lowpass linear [effect flags] |
      ffmpeg -f rawvideo -pix_fmt uyvy422 -s 720x480 -r 30000/1001 -i - -flags +ilme+ildct -field_order bb out.mpg

With a 4:2:0 `--out-pix-fmt` (yuv420p, nv12, yuv420p10le, p010le), `--out-chroma-rows interlaced` forms chroma rows 0, 2, 4, ... from the top
field's luma rows and rows 1, 3, 5, ... from the bottom field's (include/crtfx_egress_field420.h), as an interlaced decoder reads them;
without it every chroma sample of a woven frame mixes the two fields and colour combs on motion.  `--out-chroma left` then means MPEG-2's
interlaced siting.  The delivered height must be a multiple of 4 (480, 576 and 1080 are).

`--in-signal composite|svideo` sends every input frame through the cable that fed the tube (include/crtfx_signal.h): every row is encoded
to an NTSC-like signal and decoded again on the GPU, before anything else sees it — colour that bleeds sideways and, under `composite`, dot
crawl on colour edges and rainbow fringes on fine luma detail; `svideo` keeps luma and chroma apart.  One pixel is one sample at four
times the colour subcarrier (about 754 to an active line), so pass an SD-width input and let `--deliver-width` / a larger render happen
behind it.  `--signal-chroma sharp|soft` is the decoder's chroma low-pass and `--signal-crawl on|off` turns the subcarrier by 180 degrees
per frame as well as per line (on, the default: dot crawl).  NTSC-like only: no PAL, no RF noise.  A 480i capture over composite:

    ffmpeg -i capture_480i.avi -f rawvideo -pix_fmt uyvy422 - |
      python -m pythoncrt_amd.cli --input - --width 720 --height 480 --fps 60 --output - --in-pix-fmt uyvy422 \
             --in-signal composite --signal-chroma soft --deinterlace edge --deinterlace-fields both [effect flags] |
      ffmpeg -f rawvideo -pix_fmt rgb24 -s 720x480 -r 60000/1001 -i - out.mp4

`--signal-standard pal` makes that cable a PAL one (include/crtfx_pal.h) — PAL DVD, DVB, PAL-region consoles and home computers: the
subcarrier turns 270 degrees per line and per frame, the V axis switches sign every line, and the decoder averages every line's chroma with
the line above (`--pal-decoder delay`, the default) or does not (`simple`).  `--signal-phase DEGREES` (-180..180) is the decoder's phase
error: under `delay` the picture loses saturation, under `simple` it shows Hanover bars.  `ntsc` (default) is the cable as it was; NTSC has
no phase knob.  The rows of a woven frame are taken as consecutive lines; no 25 Hz offset, no RF noise.  A 576i DVD over composite:

    ffmpeg -i dvd_576i.vob -f rawvideo -pix_fmt yuv420p - |
      python -m pythoncrt_amd.cli --input - --width 720 --height 576 --fps 50 --output - --in-pix-fmt yuv420p --in-chroma-rows interlaced \
             --in-signal composite --signal-standard pal --signal-phase 15 --deinterlace edge --deinterlace-fields both [effect flags] |
      ffmpeg -f rawvideo -pix_fmt rgb24 -s 720x576 -r 50 -i - out.mp4

`--in-lut FILE` / `--deliver-lut FILE` apply a 3D colour LUT (a `.cube` file, tetrahedral interpolation; include/crtfx_lut3d.h) on the
GPU directly in front of the chain and directly behind it, at `--width x --height` and on the chain's pixels — the `lut3d=` of a second
ffmpeg process and its round trip through host memory.  `--in-lut` brings a log-encoded or HDR source to display-referred video before
the tube sees it (behind the widening of `--chain-pix half`, so an 8-bit log source is transformed at half precision); `--deliver-lut`
puts a look or display transform on the finished frames, in front of the delivery resize, the pad and the dither.  HDR10 to SDR with a
PQ / BT.2020 -> BT.709 cube of your own:

    ffmpeg -i hdr10.mkv -f rawvideo -pix_fmt p010le - |
      python -m pythoncrt_amd.cli --input - --width 3840 --height 2160 --fps 24 --output - --in-pix-fmt p010le --out-pix-fmt yuv420p \
             --chain-pix half --dither ordered --in-lut pq2020_to_709.cube [effect flags] |
      ffmpeg -f rawvideo -pix_fmt yuv420p -s 3840x2160 -r 24 -i - out.mp4

Cube sizes 2..65 and the domain 0..1 are taken; the cube's entries and the results are quarter codes (0..1020), so its precision is 10
bits.  Without the flags nothing is created and the path is as it was.

`--gui`, `--gpu`, `--nvenc-preset`, `--encoder`, `--decoder`, `--crf` and `--bitrate` are accepted for
compatibility and ignored (encode/decode/UI are not part of this path).  `--text*` rasterise the overlay on
the host with Pillow (ref:366-414) and alpha-blend it on the GPU before or after the effects.

Host staging (the reference's reader / writer pipes ref:469-514, :1003-1014, :1101): a reader thread fills pinned
input batches, a writer thread drains pinned output batches, and the GPU side runs on THREE streams — upload, kernels, download —
chained by events, so that batch k+1's upload, batch k's kernels and batch k-1's download are in flight together (the two PCIe
directions are independent DMA engines) while the host reads batch k+2 and writes batch k-2.

Regular files skip the pinned staging where the platform lets them (`--io auto`, round 5): the input file is mapped MAP_SHARED and the
windows of the mapping a batch covers are registered with the HIP runtime (hipHostRegister), so the upload DMA reads the page cache itself —
no page-cache -> pinned memcpy; the output file is sized up front (ftruncate), mapped and registered the same way and the download DMA writes
the page cache itself — no pinned -> page-cache copy.  Whether that wins depends on the filesystem (profiles/r05_hostreg_probe*.txt: on a
disk-backed filesystem registering a fresh 398 MB batch takes 4.6 ms, on tmpfs — 4 KB pages, every one marked accessed on first touch —
23-30 ms, slower than sixteen memcpy threads), so the first batch is timed and the staged path takes over when registration is refused or
slower than `_MAPPED_MIN_GBS`.  Pipes get the largest pipe buffer the kernel allows (F_SETPIPE_SZ, 1 MiB) and are read / written straight
from / to the pinned slots.
"""
from __future__ import annotations

import argparse
import itertools
import os
import sys
import time

from . import formats, tables


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="pythoncrt_amd.cli", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--input", type=str, default="")
    p.add_argument("--output", type=str)
    p.add_argument("--width", type=int, default=0)
    p.add_argument("--height", type=int, default=0)
    p.add_argument("--fps", type=int, default=0)
    p.add_argument("--scanline-strength", type=float, default=0.6)
    p.add_argument("--triad-strength", type=float, default=0.35)
    p.add_argument("--triad-gamma", type=float, default=2.2)
    p.add_argument("--triad-preserve-luma", action="store_true")
    p.add_argument("--triad-softness", type=float, default=0.5)
    p.add_argument("--aberration-px", type=int, default=1)
    p.add_argument("--bloom-sigma", type=float, default=1.2)
    p.add_argument("--bloom-strength", type=float, default=0.25)
    p.add_argument("--bloom-threshold", type=float, default=0.0)
    p.add_argument("--noise-strength", type=float, default=1.5)
    p.add_argument("--vignette-strength", type=float, default=0.25)
    p.add_argument("--persistence", type=float, default=0.2)
    p.add_argument("--crf", type=int, default=18)
    p.add_argument("--bitrate", type=int, default=0)
    p.add_argument("--scanline-speed", type=float, default=30.0)
    p.add_argument("--scanline-period", type=float, default=2.0)
    p.add_argument("--fast-bloom", action="store_true")
    p.add_argument("--no-fast-bloom", dest="fast_bloom", action="store_false")
    p.set_defaults(fast_bloom=True)
    p.add_argument("--pixel-size", type=int, default=2)
    p.add_argument("--brightness", type=float, default=0.0)
    p.add_argument("--contrast", type=float, default=1.0)
    p.add_argument("--gamma", type=float, default=1.0)
    p.add_argument("--saturation", type=float, default=1.0)
    p.add_argument("--temperature", type=float, default=0.0)
    p.add_argument("--flicker-strength", type=float, default=0.0)
    p.add_argument("--flicker-hz", type=float, default=0.0)
    p.add_argument("--grain-size", type=int, default=1)
    p.add_argument("--scanline-angle", type=float, default=0.0)
    p.add_argument("--scanline-thickness", type=float, default=1.0)
    p.add_argument("--warp-strength", type=float, default=0.0)
    p.add_argument("--text", type=str, default="")
    p.add_argument("--text-font", type=str, default="")
    p.add_argument("--text-size", type=int, default=36)
    p.add_argument("--text-color", type=str, default="#FFFFFF")
    p.add_argument("--text-x", type=int, default=32)
    p.add_argument("--text-y", type=int, default=32)
    p.add_argument("--text-after", action="store_true")
    p.add_argument("--gpu", action="store_true")
    p.add_argument("--nvenc-preset", type=str, default="p4")
    p.add_argument("--encoder", type=str, default="auto", choices=["auto", "nvidia", "amd", "cpu"])
    p.add_argument("--decoder", type=str, default="auto", choices=["auto", "nvidia", "amd", "intel", "cpu"])
    p.add_argument("--glitch-amp", type=int, default=0)
    p.add_argument("--glitch-height", type=float, default=0.0)
    p.add_argument("--gui", action="store_true")
    # not in the reference
    p.add_argument("--batch", type=int, default=16, help="frames enqueued per GPU batch")
    p.add_argument("--staging-report", action="store_true", help="print where the reader / GPU-feeding / writer threads spent their time")
    p.add_argument("--noise-seed", type=int, default=None, help="seed of the counter-based grain RNG (default: random)")
    p.add_argument("--io", type=str, default="staged", choices=["auto", "staged", "mapped"],
                   help="regular files: through pinned staging slots (staged, the default: at the PCIe rate on a disk-backed filesystem), DMA "
                        "straight from / into the registered file mapping (mapped: measured slower on this platform, profiles/r05_cli_throughput.txt), "
                        "or mapped where the first batch shows it is faster (auto)")
    return p


# the accepted formats, from the registry (pythoncrt_amd/formats.py): a 10-bit format goes on both ends or on neither (the chain then runs
# on half pixels); the 8-bit ones go on either end independently of the other
DEEP_PIX_FMTS, DEEP444_PIX_FMTS, YUV422_PIX_FMTS = formats.DEEP420.names, formats.DEEP444.names, formats.YUV422.names
OUT_PIX_FMTS = IN_PIX_FMTS = formats.PIX_FMTS


def add_output_flags(p: argparse.ArgumentParser) -> argparse.ArgumentParser:
    """The output-format flags of `main` (not in the reference, whose encoder pipe is always rgb24 in and `-pix_fmt yuv420p` out, ref:970-1002).
    Kept out of `build_parser`, which restates the reference's schema plus the four additions listed there."""
    p.add_argument("--out-pix-fmt", type=str, default="rgb24", choices=list(OUT_PIX_FMTS),
                   help="format of the frames written: raw rgb24 (default), or planar yuv420p / semi-planar nv12 converted on the GPU (1.5 bytes per pixel); "
                        "planar yuv422p / packed yuyv422 / uyvy422 (2 bytes per pixel); "
                        "yuv420p10le / p010le (3 bytes per pixel) or yuv444p10le / gbrp10le (6) / x2rgb10le (4) with a 10-bit --in-pix-fmt: the chain "
                        "then runs on half pixels")
    p.add_argument("--out-matrix", type=str, default="bt601", choices=["bt601", "bt709"], help="yuv420p / nv12 / 4:2:2: the RGB -> Y'CbCr matrix")
    p.add_argument("--out-range", type=str, default="tv", choices=["tv", "pc"], help="yuv420p / nv12 / 4:2:2: limited (tv, 16-235) or full (pc) range")
    p.add_argument("--out-chroma", type=str, default="center", choices=["center", "left"],
                   help="4:2:0 / 4:2:2 output: write chroma as the box mean of its pixels (center, default: ffprobe's chroma_location=center), or filter it "
                        "onto its first luma column on the GPU (left: MPEG-2 / H.264 / HEVC and every 4:2:2 format; ffprobe's chroma_location=left or nothing)")
    p.add_argument("--deliver-width", type=int, default=0,
                   help="width of the frames written, with --deliver-height: the frames are rendered at --width x --height and resized on the GPU behind "
                        "the chain (a 4K render written as 1080p); 0 (default) = as rendered")
    p.add_argument("--deliver-height", type=int, default=0, help="height of the frames written (see --deliver-width); 0 (default) = as rendered")
    p.add_argument("--deliver-filter", type=str, default="bilinear", choices=list(tables.RESAMPLE_FILTERS),
                   help="filter of the --deliver-width / --deliver-height resize: Pillow's BILINEAR (default) or another of its five, e.g. lanczos or "
                        "bicubic for a 4K render written as 1080p; needs a delivery size other than the render size")
    p.add_argument("--deliver-fit", type=str, default="stretch", choices=["stretch", "pad", "crop"],
                   help="how the render meets a --deliver-width x --deliver-height of another aspect: stretch it (default), pad: resize it to fit "
                        "inside and centre it on a frame of --deliver-pad-color (a 4:3 render pillarboxed in 16:9), or crop: cut the centred window "
                        "of the delivery's aspect and resize that; on the GPU (include/crtfx_canvas.h); needs a delivery size other than the render size")
    p.add_argument("--deliver-pad-color", type=str, default="0,0,0", help="R,G,B of the bars of --deliver-fit pad, each 0..255 (default 0,0,0)")
    p.add_argument("--chain-pix", type=str, default="auto", choices=["auto", "half"],
                   help="what the chain runs on: what the formats say (auto, default: uint8 pixels, or half ones between two 10-bit formats), or half "
                        "pixels whatever the formats (half): an 8-bit input is widened and an 8-bit output narrowed on the GPU "
                        "(include/crtfx_depth.h), so a 10-bit format may stand on one end only")
    p.add_argument("--dither", type=str, default="none", choices=["none", "ordered"],
                   help="how --chain-pix half narrows its half frames to an 8-bit output: round to nearest (none, default) or 8 x 8 ordered (Bayer) "
                        "dither at the delivered frame's coordinates (ordered); needs --chain-pix half and an 8-bit or rgb24 --out-pix-fmt")
    p.add_argument("--deliver-lut", type=str, default="", metavar="FILE",
                   help="a .cube file (3D LUT, sizes 2..65, domain 0..1) applied to the finished frames on the GPU, directly behind the chain and in "
                        "front of the delivery resize, the pad and the dither (include/crtfx_lut3d.h: tetrahedral, 10-bit entries); default: none")
    p.add_argument("--deliver-interlace", type=str, default="off", choices=["off", "tff", "bff"],
                   help="weave every two consecutive finished frames into one interlaced frame on the GPU (include/crtfx_interlace.h), behind the "
                        "delivery resize and the pad and in front of the dither and the output format: the first frame of a pair gives the even rows "
                        "(tff) or the odd rows (bff); the output holds half the frames, an odd last one woven with itself (pass the field rate as "
                        "--fps); off (default) = a progressive delivery")
    p.add_argument("--deliver-lowpass", type=str, default="none", choices=["none", "linear", "complex"],
                   help="vertical low-pass of every row inside its own frame before the weave, against line twitter: [1 2 1] / 4 (linear) or "
                        "[-1 2 6 2 -1] / 8 held back from over-sharpening (complex); none (default) copies rows; needs --deliver-interlace")
    p.add_argument("--out-chroma-rows", type=str, default="progressive", choices=["progressive", "interlaced"],
                   help="which luma rows a chroma row of a 4:2:0 --out-pix-fmt is formed from: rows 2c and 2c + 1, one of each field (progressive, "
                        "default), or rows of the chroma row's own field only, as an interlaced decoder reads them (interlaced: "
                        "include/crtfx_egress_field420.h; --out-chroma left is then MPEG-2's interlaced siting; the delivered height must be a "
                        "multiple of 4)")
    return p


def luts_from_args(a):
    """(in cube | None, delivery cube | None) of --in-lut / --deliver-lut, read once per parsed command line."""
    if getattr(a, "_luts", None) is None:
        from .cube import as_cube
        cubes = []
        for flag, path in (("--in-lut", getattr(a, "in_lut", "")), ("--deliver-lut", getattr(a, "deliver_lut", ""))):
            try:
                cubes.append(as_cube(path, flag) if path else None)
            except ValueError as e:
                raise SystemExit(f"{flag}: {e}") from None
        a._luts = tuple(cubes)
    return a._luts


def deliver_size_from_args(a):
    """(dh, dw) of --deliver-height / --deliver-width, or None where the frames are written as rendered.  Both flags, or neither."""
    dw, dh = int(getattr(a, "deliver_width", 0) or 0), int(getattr(a, "deliver_height", 0) or 0)
    if (dw == 0) != (dh == 0):
        raise SystemExit("--deliver-width and --deliver-height go together: pass both, or neither (0 = as rendered)")
    if dw == 0:
        return None
    if min(dh, dw) < 1 or max(dh, dw) > 32767:
        raise SystemExit(f"--deliver-width {dw} --deliver-height {dh}: sizes outside 1..32767")
    return None if (dh, dw) == (int(a.height), int(a.width)) else (dh, dw)


def pad_color_from_args(a):
    """(r, g, b) of --deliver-pad-color."""
    text = str(getattr(a, "deliver_pad_color", "0,0,0"))
    try:
        vals = tuple(int(v) for v in text.split(","))
    except ValueError:
        vals = ()
    if len(vals) != 3 or min(vals) < 0 or max(vals) > 255:
        raise SystemExit(f"--deliver-pad-color {text}: three integers R,G,B in 0..255")
    return vals


def in_crop_from_args(a):
    """(y, x, h, w) of --in-crop-y / -x / -height / -width, or None.  A window needs both sides; 0 (default) everywhere = none."""
    x, y, cw, ch = (int(getattr(a, "in_crop_" + k, 0) or 0) for k in ("x", "y", "width", "height"))
    if (cw == 0) != (ch == 0) or (cw == 0 and (x or y)):
        raise SystemExit("--in-crop-x, --in-crop-y, --in-crop-width and --in-crop-height go together: pass a window with both sides, or none of them "
                         "(0 = no crop)")
    if cw == 0:
        return None
    if min(cw, ch) < 1 or min(x, y) < 0 or x + cw > int(a.width) or y + ch > int(a.height):
        raise SystemExit(f"--in-crop-x {x} --in-crop-y {y} --in-crop-width {cw} --in-crop-height {ch}: the window leaves the "
                         f"--width {a.width} x --height {a.height} input")
    return y, x, ch, cw


def add_input_flags(p: argparse.ArgumentParser) -> argparse.ArgumentParser:
    """The input-format flags of `main` (not in the reference, whose reader pipe is always `-pix_fmt rgb24`, ref:489-502).  Kept out of
    `build_parser`, as `add_output_flags` is."""
    p.add_argument("--in-pix-fmt", type=str, default="rgb24", choices=list(IN_PIX_FMTS),
                   help="format of the frames read: raw rgb24 (default), or planar yuv420p / semi-planar nv12 converted on the GPU (1.5 bytes per pixel); "
                        "planar yuv422p / packed yuyv422 / uyvy422 (2 bytes per pixel); "
                        "yuv420p10le / p010le (3 bytes per pixel) or yuv444p10le / gbrp10le (6) / x2rgb10le (4) with a 10-bit --out-pix-fmt: the chain "
                        "then runs on half pixels")
    p.add_argument("--in-matrix", type=str, default="bt601", choices=["bt601", "bt709"], help="yuv420p / nv12 / 4:2:2 input: the Y'CbCr -> RGB matrix")
    p.add_argument("--in-range", type=str, default="tv", choices=["tv", "pc"], help="yuv420p / nv12 / 4:2:2 input: limited (tv, 16-235) or full (pc) range")
    p.add_argument("--in-chroma", type=str, default="replicate", choices=["replicate", "left", "center"],
                   help="4:2:0 / 4:2:2 input: replicate each chroma sample over its pixels (default), or interpolate chroma at its siting on the GPU: "
                        "left (MPEG-2 / H.264 / HEVC; ffprobe's chroma_location=left or nothing) or center (JPEG-family sources)")
    p.add_argument("--in-chroma-rows", type=str, default="progressive", choices=["progressive", "interlaced"],
                   help="yuv420p / nv12 / yuv420p10le / p010le input: progressive (default) pairs chroma row c with luma rows 2c and 2c + 1; interlaced reads "
                        "what an interlaced encoder wrote (DVD, 480i / 576i / 1080i broadcast): chroma rows alternate between the fields and every luma "
                        "row takes colour from rows of its own field on the GPU (include/crtfx_field420.h), at --in-chroma; pass it with --deinterlace")
    p.add_argument("--in-filter", type=str, default="bilinear", choices=list(tables.RESAMPLE_FILTERS),
                   help="filter of the resize that brings a source of another size to --width x --height (process_frames(in_filter=)): Pillow's "
                        "BILINEAR (default) or another of its five; a raw input file is read at --width x --height, so nothing is resized in "
                        "front of the chain here")
    p.add_argument("--in-crop-x", type=int, default=0,
                   help="left column of a window of the --width x --height input that is cut out on the GPU (include/crtfx_canvas.h) and resized back "
                        "to --width x --height for the render (a letterboxed source: the picture area fills the tube); with --in-crop-y, "
                        "--in-crop-width and --in-crop-height; all 0 (default) = no crop")
    p.add_argument("--in-crop-y", type=int, default=0, help="top row of the window (see --in-crop-x)")
    p.add_argument("--in-crop-width", type=int, default=0, help="width of the window (see --in-crop-x); 0 (default) = no crop")
    p.add_argument("--in-crop-height", type=int, default=0, help="height of the window (see --in-crop-x); 0 (default) = no crop")
    p.add_argument("--deinterlace", type=str, default="off", choices=["off", "linear", "edge", "adaptive"],
                   help="take every input frame as two fields woven into its even and odd rows and deinterlace it on the GPU, in front of the crop "
                        "and the resize (include/crtfx_deint.h): the rows between a field's rows are the mean of the rows above and below (linear) "
                        "or of two of their pixels along the best of five directions per pixel (edge); adaptive (include/crtfx_adeint.h) keeps the "
                        "other field's rows where the picture did not change since the previous frame and takes edge's where it did; off (default) "
                        "= a progressive input")
    p.add_argument("--field-order", type=str, default="tff", choices=["tff", "bff"],
                   help="which field of an interlaced input comes first: the even rows (tff, default) or the odd rows (bff); needs --deinterlace")
    p.add_argument("--deinterlace-fields", type=str, default="first", choices=["first", "both"],
                   help="write one frame per input frame, made for its first field (first, default), or one per field in field order (both: twice "
                        "the frames; pass the field rate as --fps); needs --deinterlace")
    p.add_argument("--in-lut", type=str, default="", metavar="FILE",
                   help="a .cube file (3D LUT, sizes 2..65, domain 0..1) applied to the source frames on the GPU at --width x --height, directly in "
                        "front of the chain: behind the resize and, under --chain-pix half, behind the widening (include/crtfx_lut3d.h: "
                        "tetrahedral, 10-bit entries) — log footage or HDR10 brought to display-referred video; default: none")
    p.add_argument("--in-signal", type=str, default="rgb", choices=["rgb", "composite", "svideo"],
                   help="send every input frame through an NTSC-like composite or S-Video encode and decode on the GPU (include/crtfx_signal.h), at "
                        "the input's size and in front of the deinterlacer, the crop and the resize: colour bleed and, under composite, dot crawl "
                        "and rainbow fringes; one pixel is one sample at four times the colour subcarrier, so pass an SD-width input; rgb (default) "
                        "= no signal")
    p.add_argument("--signal-chroma", type=str, default="sharp", choices=["sharp", "soft"],
                   help="the decoder's chroma low-pass under --in-signal: [1 2 3 4 3 2 1] / 16 (sharp, default) or [1 2 .. 8 .. 2 1] / 64 (soft)")
    p.add_argument("--signal-crawl", type=str, default="on", choices=["on", "off"],
                   help="turn the subcarrier by 180 degrees per frame as well as per line (on, default: dot crawl) or per line only (off); needs "
                        "--in-signal")
    p.add_argument("--signal-standard", type=str, default="ntsc", choices=["ntsc", "pal"],
                   help="the colour standard of --in-signal: ntsc (default: include/crtfx_signal.h, 180 degrees per line) or pal "
                        "(include/crtfx_pal.h: 270 degrees per line, the V switch and a delay-line decoder — 576i sources); needs --in-signal")
    p.add_argument("--pal-decoder", type=str, default="delay", choices=["delay", "simple"],
                   help="the PAL decoder: delay (default) averages every line's chroma with the line above, simple does not (a phase error "
                        "then shows as Hanover bars); needs --signal-standard pal")
    p.add_argument("--signal-phase", type=int, default=0, metavar="DEGREES",
                   help="the PAL decoder's phase error in whole degrees, -180..180 (default 0); needs --signal-standard pal")
    return p


def settings_from_args(a):
    """The clamps of main() (ref:1225-1266) -> RenderSettings."""
    from .pipeline import RenderSettings
    return RenderSettings(
        scanline_strength=float(max(0.0, min(1.0, a.scanline_strength))),
        triad_strength=float(max(0.0, min(1.0, a.triad_strength))),
        triad_gamma=float(max(0.1, a.triad_gamma)),
        triad_preserve_luma=bool(a.triad_preserve_luma),
        triad_softness=float(max(0.0, a.triad_softness)),
        aberration_px=int(max(-8, min(8, a.aberration_px))),
        bloom_sigma=max(0.0, a.bloom_sigma),
        bloom_strength=max(0.0, a.bloom_strength),
        noise_strength=max(0.0, a.noise_strength),
        vignette_strength=float(max(0.0, min(1.0, a.vignette_strength))),
        persistence=float(max(0.0, min(0.95, a.persistence))),
        scanline_speed_px_s=float(a.scanline_speed),
        scanline_period_px=max(1.0, float(a.scanline_period)),
        fast_bloom=bool(a.fast_bloom),
        pixel_size=max(1, int(a.pixel_size)),
        glitch_amp_px=max(0, int(a.glitch_amp)),
        glitch_height_frac=float(max(0.0, min(1.0, a.glitch_height))),
        bloom_threshold=float(max(0.0, min(1.0, a.bloom_threshold))),
        brightness=float(a.brightness),
        contrast=float(a.contrast),
        gamma=float(max(1e-3, a.gamma)),
        saturation=float(max(0.0, a.saturation)),
        temperature=float(max(-1.0, min(1.0, a.temperature))),
        flicker_strength=float(max(0.0, min(1.0, a.flicker_strength))),
        flicker_hz=float(max(0.0, a.flicker_hz)),
        grain_size=max(1, int(a.grain_size)),
        scanline_angle=float(a.scanline_angle),
        scanline_thickness=float(max(0.1, a.scanline_thickness)),
        warp_strength=float(max(-1.0, min(1.0, a.warp_strength))),
    )


def main_sharded(a, spec, rank: int, world: int) -> int:
    """One process per GPU (launched with `python -m torch.distributed.run --nproc-per-node N -m pythoncrt_amd.cli ...`):
    the clip's chunks of --batch frames are dealt round-robin over the ranks, each rank reads its chunks
    from the raw input file and writes them at the same offsets of the output file; with --persistence > 0 one
    float32 state frame per chunk boundary travels to the next rank (RCCL)."""
    if getattr(a, "chain_pix", "auto") != "auto":
        raise SystemExit(f"--chain-pix {a.chain_pix} (and with it --dither) is not supported by the sharded CLI (one process per GPU reads and writes "
                         "rgb24 on a uint8 chain); run one process")
    if getattr(a, "deliver_width", 0) or getattr(a, "deliver_height", 0):
        # every rank writes its chunks at offsets of its own: those, and the downloads behind them, are at render size here
        raise SystemExit("--deliver-width / --deliver-height are not supported by the sharded CLI (one process per GPU writes rgb24 at render size); "
                         "run one process, or scale behind it")
    for flag, on in (("--in-crop-x / --in-crop-y / --in-crop-width / --in-crop-height", any(getattr(a, "in_crop_" + k, 0) for k in ("x", "y", "width", "height"))),
                     ("--deinterlace / --field-order / --deinterlace-fields", spec.deinterlace is not None),
                     ("--in-signal / --signal-chroma / --signal-crawl", spec.signal is not None),
                     ("--in-lut", bool(getattr(a, "in_lut", ""))), ("--deliver-lut", bool(getattr(a, "deliver_lut", ""))),
                     ("--deliver-interlace / --deliver-lowpass", spec.weave is not None),
                     ("--deliver-fit", getattr(a, "deliver_fit", "stretch") != "stretch"),
                     ("--deliver-pad-color", str(getattr(a, "deliver_pad_color", "0,0,0")) != "0,0,0")):
        if on:
            raise SystemExit(f"{flag} is not supported by the sharded CLI (one process per GPU reads and writes rgb24 at render size); "
                             "run one process, or crop / pad outside it")
    for flag, value in (("--in-filter", getattr(a, "in_filter", "bilinear")), ("--deliver-filter", getattr(a, "deliver_filter", "bilinear"))):
        if value != "bilinear":
            raise SystemExit(f"{flag} {value} is not supported by the sharded CLI (one process per GPU reads and writes rgb24 at render size: "
                             "nothing is resized); run one process, or scale outside it")
    if getattr(a, "out_pix_fmt", "rgb24") != "rgb24":
        # every rank writes its chunks at offsets of its own: those, and the downloads behind them, are rgb24-sized here
        raise SystemExit(f"--out-pix-fmt {a.out_pix_fmt} is not supported by the sharded CLI (one process per GPU writes rgb24 only); "
                         "run one process, or convert behind it")
    if getattr(a, "in_pix_fmt", "rgb24") != "rgb24":
        # every rank reads its chunks at offsets of its own: those, and the uploads behind them, are rgb24-sized here
        raise SystemExit(f"--in-pix-fmt {a.in_pix_fmt} is not supported by the sharded CLI (one process per GPU reads rgb24 only); "
                         "run one process, or convert in front of it")
    import torch
    import torch.distributed as dist
    from .pipeline import FramePipeline, GpuShardEngine
    from .shard import FrameShard, ShardedRender
    from .staging import _Reader, _Writer
    from .text import make_text_overlay_rgba
    if a.input == "-" or not a.output or a.output == "-":
        raise SystemExit("the sharded CLI needs seekable --input and --output files")
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device visible; pythoncrt_amd has no CPU fallback")
    ndev = torch.cuda.device_count()
    local_rank = int(os.environ.get("LOCAL_RANK", rank))
    dev = torch.device("cuda", local_rank % ndev)
    torch.cuda.set_device(dev)
    backend = os.environ.get("CRTFX_DIST_BACKEND", "nccl" if ndev >= world else "gloo")     # gloo: rehearsal of N ranks on fewer GPUs
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if "MASTER_PORT" not in os.environ:                  # CRTFX_FORCE_DIST=1 without a launcher
        import socket
        with socket.socket() as s_:
            s_.bind(("127.0.0.1", 0))
            os.environ["MASTER_PORT"] = str(s_.getsockname()[1])
    dist.init_process_group(backend, rank=rank, world_size=world, **({"device_id": dev} if backend == "nccl" else {}))
    rs = settings_from_args(a)
    fps_out = int(a.fps) if a.fps and a.fps > 0 else 24
    h, w = int(a.height), int(a.width)
    box = [a.noise_seed if a.noise_seed is not None else int.from_bytes(os.urandom(8), "little")]
    dist.broadcast_object_list(box, src=0)               # every rank draws the same grain stream
    overlay = make_text_overlay_rgba(w, h, a.text, a.text_font, a.text_size, a.text_color, (a.text_x, a.text_y)) if a.text else None
    pipe = FramePipeline(dev, h, w, rs, fps=fps_out, noise_seed=box[0], text_overlay_rgba=overlay, text_overlay_after=bool(a.text_after))
    B = max(1, int(a.batch))
    frame_bytes = h * w * 3
    n_frames = os.path.getsize(a.input) // frame_bytes
    shard = FrameShard(world, rank, B)
    # overlapped schedule where the chunk covers the IIR's settling time (shard.py): round r's state frame travels while round
    # r+1 is scanned, results come back one call late; any other case runs the synchronous protocol behind the same calls
    # — over gloo (rehearsals).  Over RCCL the synchronous hop stays the default until the overlapped one has run on a multi-GPU
    # box (it costs ~0.3 ms per round: one state frame over one xGMI link + the fix-up); CRTFX_SHARD_OVERLAP=1 opts in.
    ov = os.environ.get("CRTFX_SHARD_OVERLAP")            # "1" / "0": force the overlapped / the synchronous schedule (tests run both over gloo)
    overlap = (ov == "1") if ov in ("0", "1") else backend == "gloo"
    # test hook: hold every download back by this many milliseconds of GPU time, so that a missing ordering between a round's download and the
    # next round's kernels shows as wrong bytes instead of passing by timing (tests/test_cli_gpu.py::test_sharded_cli_synchronous_schedule)
    down_delay_ms = float(os.environ.get("CRTFX_TEST_DOWNLOAD_DELAY_MS", "0") or 0)
    # three output slots: round r's frames may still be on their way to the host (download stream) while round r + 1 is scanned and —
    # overlapped schedule, results one call late — round r + 2 is enqueued
    # world 1 arrives here only as CRTFX_FORCE_DIST=1 (main): the one-rank ring — the same protocol with rank 0 as its own neighbour, so that
    # this function's RCCL branch (eager communicator, object broadcast, the hop between the three streams below) runs on a one-GPU box
    render = ShardedRender(shard, rs.persistence, GpuShardEngine(pipe, B, slots=3), dist=dist, overlap=overlap, loopback=(world == 1))
    if rank == 0:
        with open(a.output, "wb") as f:
            f.truncate(n_frames * frame_bytes)
    dist.barrier()
    t0 = time.perf_counter()
    fin, fout = open(a.input, "rb", buffering=0), open(a.output, "r+b", buffering=0)
    n_rounds = shard.rounds(n_frames)
    mine = [(r,) + shard.frame_range(r, n_frames) for r in range(n_rounds)]
    reader = _Reader(fin, True, ((lo * frame_bytes, hi - lo) for _, lo, hi in mine if hi > lo), (B, h, w, 3), frame_bytes, slots=2)
    writer = _Writer(fout, True, (B, h, w, 3), frame_bytes, slots=2)
    compute = torch.cuda.current_stream(dev)
    s_up, s_down = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    dev_in = [torch.empty((B, h, w, 3), dtype=torch.uint8, device=dev) for _ in range(2)]
    in_free = [None, None]                                # per device input slot: the event after which the kernels no longer read it
    downs = []                                            # download events in order of issue

    def commit(finished):
        for rr, out in finished:
            flo, fhi = shard.frame_range(rr, n_frames)
            n = fhi - flo
            i = writer.slot()
            ready = torch.cuda.Event()
            ready.record(compute)                         # the round's kernels (and fix-up) are enqueued behind this point at the latest
            s_down.wait_event(ready)
            with torch.cuda.stream(s_down):
                if down_delay_ms > 0:
                    torch.cuda._sleep(int(down_delay_ms * 2.0e6))      # ~2 GHz shader clock; the exact length does not matter
                writer.bufs[i][:n].copy_(out[:n], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(s_down)
            downs.append(ev)
            writer.put(i, n, ev, flo * frame_bytes)

    k, pend = 0, None
    for r, lo, hi in mine:
        frames = None
        if hi > lo:
            item = reader.get()
            if item is None or item[1] != hi - lo:
                raise SystemExit(f"short read at frame {lo}")
            i, n, _ = item
            d = k & 1
            if in_free[d] is not None:
                s_up.wait_event(in_free[d])               # the kernels that read this device slot two rounds ago are done
            with torch.cuda.stream(s_up):
                dev_in[d][:n].copy_(reader.bufs[i][:n], non_blocking=True)
                up = torch.cuda.Event()
                up.record(s_up)
            compute.wait_event(up)
            frames = dev_in[d][:n]
            k += 1
        # the engine's three output slots come round every third round: every download but the latest must have left them
        for ev in downs[:-1]:
            compute.wait_event(ev)
        del downs[:-1]
        commit(render.submit_round(frames, r, active=shard.active_ranks(r, n_frames)))
        if pend is not None:                              # the previous chunk's pinned slot: free again once its upload has completed (long done)
            pend[0].synchronize()
            reader.release(pend[1])
            pend = None
        if hi > lo:
            pend = (up, i)
            ev = torch.cuda.Event()
            ev.record(compute)                            # the scan that reads dev_in[d] is enqueued by now (the fix-up reads local states only)
            in_free[d] = ev
    if pend is not None:
        pend[0].synchronize()
        reader.release(pend[1])
    commit(render.close())                                # the round still in flight; frees the staged schedule's extra process groups
    writer.close()
    reader.close()
    done = writer.frames
    fin.close(); fout.close()
    dist.barrier()
    print(f"rank {rank}: {done} of {n_frames} frames, elapsed {time.perf_counter() - t0:.3f}s", file=sys.stderr)
    dist.destroy_process_group()
    return 0


def check_flags(a):
    """Every refusal from the flags alone, before torch, a device or the output file: options.RULES in their flag wording, around the parsers
    of the CLI's own syntax.  -> the ChainOptions, (rank, world) | None.  For the sharded CLI only the rules in front of its branch have run:
    it refuses a crop, a pad colour and a cube itself, and its spec holds none."""
    from .options import ChainOptions, OptionError, Raw, refuse
    hw = (a.height if a.height > 0 else None, a.width if a.width > 0 else None)        # None: not given (refused below, behind the sharded branch)
    v = Raw(render_hw=hw, in_size=hw, resize_on="device", in_pix_fmt=a.in_pix_fmt, in_matrix=a.in_matrix, in_range=a.in_range, in_chroma=a.in_chroma,
            in_filter=a.in_filter, in_crop=None, deinterlace=a.deinterlace, field_order=a.field_order, deinterlace_fields=a.deinterlace_fields,
            in_signal=a.in_signal, signal_chroma=a.signal_chroma, signal_crawl=a.signal_crawl == "on", in_lut=None, chain_pix=a.chain_pix,
            dither=a.dither, out_pix_fmt=a.out_pix_fmt, out_matrix=a.out_matrix, out_range=a.out_range, out_chroma=a.out_chroma,
            deliver_size=deliver_size_from_args(a), deliver_filter=a.deliver_filter, deliver_fit=a.deliver_fit, deliver_pad_color=(0, 0, 0),
            deliver_lut=None, deliver_interlace=a.deliver_interlace, deliver_lowpass=a.deliver_lowpass, in_chroma_rows=a.in_chroma_rows,
            out_chroma_rows=a.out_chroma_rows, signal_standard=a.signal_standard, pal_decoder=a.pal_decoder, signal_phase=a.signal_phase)
    try:
        refuse(v, "flags", early=True)
        if int(os.environ.get("WORLD_SIZE", "1")) > 1 or os.environ.get("CRTFX_FORCE_DIST") == "1":
            if a.gui or not a.input or a.width <= 0 or a.height <= 0:
                raise SystemExit("pass --input, --width and --height")
            return ChainOptions.build(v), (int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")))
        v.deliver_pad_color = pad_color_from_args(a)
        if a.gui or not a.input:
            raise SystemExit("the GUI is not part of this path; pass --input (raw rgb24 / yuv420p / nv12 / yuv422p / yuyv422 / uyvy422 / yuv420p10le / p010le / yuv444p10le / gbrp10le / x2rgb10le file or '-')")
        if a.width <= 0 or a.height <= 0:
            raise SystemExit("raw input needs --width and --height")
        v.in_crop = in_crop_from_args(a)
        refuse(v, "flags", early=False)
    except OptionError as e:
        raise SystemExit(str(e)) from e
    v.in_lut, v.deliver_lut = luts_from_args(a)                    # an unreadable or malformed cube
    return ChainOptions.build(v), None


def open_output(a, fin, out_path: str, B: int, in_bytes: int, out_bytes: int, ratio: int = 1, frames=None):
    """Open the output.  -> it, is each end a regular file (positional I/O; else sequential)?, pipe buffer sizes, [(offset, bytes)] per batch | None.
    `B` counts the chain's frames per batch, `ratio` of them per input frame (2 under --deinterlace-fields both; B is then even).  `frames`
    (DeliveryEnd.frames) gives the frames delivered for a batch of the chain's: under --deliver-interlace half of them, an odd last batch
    rounded up (B is then even, so only the last batch can be odd)."""
    from .staging import _grow_pipe, _seekable
    in_pos = _seekable(fin) and a.input != "-"
    # opened with read access too (a MAP_SHARED, PROT_WRITE mapping needs O_RDWR).  --io mapped | auto only: an existing regular output behind a regular
    # input is NOT truncated at open but sized to the clip below, its cached pages overwritten (registering them is several times faster than allocating).
    # The default truncates and the file GROWS: a render that dies leaves a short file, never frames of an earlier render (the sized paths: abandon).
    if in_pos and out_path != "-" and os.path.exists(out_path) and os.path.samefile(out_path, a.input):
        raise SystemExit("--output is the input file")
    presize = in_pos and out_path != "-" and a.io in ("mapped", "auto")
    keep_pages = presize and os.path.isfile(out_path)
    fout = sys.stdout.buffer if out_path == "-" else open(out_path, "r+b" if keep_pages else "w+b")
    out_pos = fout is not sys.stdout.buffer and _seekable(fout)
    pipes = (0 if in_pos else _grow_pipe(fin)), (0 if out_pos else _grow_pipe(fout))      # pipes: the largest buffer the kernel allows
    # a regular input file fixes the output file's size: it can be sized, mapped and registered up front (a stream's goes through the pinned slots)
    out_plan = None
    if in_pos and out_pos:
        n_total = os.fstat(fin.fileno()).st_size // in_bytes * ratio
        frames = frames or (lambda m: m)
        out_plan = [(k * frames(B) * out_bytes, frames(min(B, n_total - k * B)) * out_bytes) for k in range((n_total + B - 1) // B)] or None
        if presize and out_pos:
            os.ftruncate(fout.fileno(), (out_plan[-1][0] + out_plan[-1][1]) if out_plan else 0)
    return fout, in_pos, out_pos, pipes, out_plan


def feed(pipe, source, end, reader, writer, NS: int, fout, timed: bool):
    """The feed loop: every batch of the reader is uploaded, run through [source] -> chain -> [delivery end] and downloaded to the writer, on three
    streams chained by events.  `fout`: the output if a regular file.  Returns the frames delivered, the timing events, the seconds per leg.
    The reader's batches count input frames; a source that deinterlaces to both fields (source.ratio = 2) makes two chain frames of each, and
    the frame indices count those.  The writer and the return value count DELIVERED frames: end.frames(m) of a batch of m chain frames, which
    is m unless the delivery end interlaces."""
    import torch
    dev, Bs, in_bytes, out_bytes = pipe.device, reader.shape[0], reader.frame_bytes, end.frame_bytes
    ratio = 1 if source is None else source.ratio
    B = Bs * ratio
    reader.start()
    if source is not None:
        source.restart()                                            # a new stream: --deinterlace adaptive starts without a previous frame
    dev_in, dev_out = ([torch.empty((B, pipe.h, pipe.w, 3), dtype=pipe.dtype, device=dev) for _ in range(NS)] for _ in range(2))
    dev_recv = dev_in if source is None else source.slots(Bs, NS, pinned=False).dev        # what is uploaded
    end.slots(dev_out)                                              # what the egress plan reads, what is downloaded
    compute, s_up, s_down = torch.cuda.current_stream(dev), torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    kernels_done, down_done = [None] * NS, [None] * NS      # per device slot: its batch's kernels (dev_in free again) / download (dev_out free again)
    state, index, delivered, k, out_off, pend, marks = None, 0, 0, 0, 0, None, []
    t_get = t_enq = t_slot = t_rel = 0.0

    def mark(stream, timing=timed):
        ev = torch.cuda.Event(enable_timing=timing)
        ev.record(stream)
        return ev
    try:
        while True:
            tt = time.perf_counter()
            item = reader.get()
            t_get += time.perf_counter() - tt
            if item is None:
                break
            i, n, got = item                                            # a trailing partial frame is dropped, as ffmpeg's rawvideo demuxer does
            m = n * ratio                                               # the frames the chain runs
            md = end.frames(m)                                          # the frames the writer gets
            tt = time.perf_counter()
            if n:
                d = k % NS
                # upload k on its own stream, once the kernels that last read this device slot (batch k - NS) are done
                if kernels_done[d] is not None:
                    s_up.wait_event(kernels_done[d])
                u0 = mark(s_up) if timed else None
                reader.upload(i, n, dev_recv[d], s_up)            # from the pinned slot, or straight from the registered file mapping
                up = mark(s_up)
                # kernels k behind the upload, and behind the download that last read this output slot
                compute.wait_event(up)
                if down_done[d] is not None:
                    compute.wait_event(down_done[d])
                k0 = mark(compute) if timed else None
                # on the compute stream and counted with the kernels (k0 ... kd): dev_in[d]'s last reader (batch k - NS) ran on this stream
                if source is not None:
                    source.index = index // ratio                    # the batch's first input frame in the stream: --in-signal's t
                    source.convert(d, n, dev_in[d][:m])
                _, state = pipe.run(dev_in[d][:m], first_index=index, state=state, out=dev_out[d][:m])
                send = end.run(d, m)
                kd = mark(compute)
                kernels_done[d] = kd
                # download k on the third stream into a free pinned slot; the writer thread takes it from there
                t_enq += time.perf_counter() - tt
                tt = time.perf_counter()
                j = writer.slot()
                t_slot += time.perf_counter() - tt
                tt = time.perf_counter()
                s_down.wait_event(kd)
                d0 = mark(s_down) if timed else None
                writer.download(j, md, send, s_down)               # into the pinned slot, or straight into the registered output mapping
                dn = mark(s_down)
                down_done[d] = dn
                if timed:
                    marks.append((u0, up, k0, kd, d0, dn, n, md))
                writer.put(j, md, dn, out_off if fout is not None else None)
                out_off += md * out_bytes
            # a pinned input slot goes back once its upload has completed: the PREVIOUS batch's (long done), never the one just enqueued
            t_enq += time.perf_counter() - tt
            tt = time.perf_counter()
            if pend is not None:
                pend[0].synchronize()
                reader.release(pend[1])
                pend = None
            t_rel += time.perf_counter() - tt
            if n:
                pend = (up, i)
            else:
                reader.release(i)
            index += m
            delivered += md
            k += 1
            if got < Bs * in_bytes:
                break
        if pend is not None:
            pend[0].synchronize()
            reader.release(pend[1])
        writer.close()
    except BaseException:
        abandon(dev, reader, writer, fout, delivered, out_bytes)
        raise
    return delivered, marks, (t_get, t_enq, t_slot, t_rel)


def abandon(dev, reader, writer, fout, index: int, out_bytes: int) -> None:
    """The render died: the GPU is drained, the writer stopped, a regular output file `fout` cut back to the frames written (a prefix).
    `index` counts delivered frames, as the writer does."""
    import contextlib
    import torch
    with contextlib.suppress(Exception):
        torch.cuda.synchronize(dev)
    for close in (writer.close, reader.close):
        with contextlib.suppress(BaseException):    # the first error is the one to report
            close()
    if fout is not None:
        with contextlib.suppress(OSError):
            fout.flush()
            os.ftruncate(fout.fileno(), min(int(writer.frames), index) * out_bytes)


def staging_report(index: int, marks, waits, times, reader, writer, pipes) -> None:
    """The lines of --staging-report: the GPU side per batch from the timing events, then where the three host threads spent their time."""
    import torch
    (t_pipe, t_imports, t_engine, t_slots), in_bytes, out_bytes = times, reader.frame_bytes, writer.frame_bytes
    if len(marks) > 4:
        torch.cuda.synchronize()
        mk = marks[2:]                   # past the start-up batches
        up_ms, k_ms, dn_ms = (sum(m[i].elapsed_time(m[i + 1]) for m in mk) / len(mk) for i in (0, 2, 4))
        span = mk[0][0].elapsed_time(mk[-1][5]) / len(mk)
        nf = sum(m[6] for m in mk) / len(mk)
        nb, nb_out = nf * in_bytes, sum(m[7] for m in mk) / len(mk) * out_bytes       # frames read, frames written (two per frame read under --deinterlace-fields both)
        print(f"staging (GPU side, per batch of {nf:.0f} frames): upload {up_ms:.2f} ms = {nb / up_ms / 1e6:.1f} GB/s, kernels {k_ms:.2f} ms, "
              f"download {dn_ms:.2f} ms = {nb_out / dn_ms / 1e6:.1f} GB/s; one batch every {span:.2f} ms = {nf / span * 1e3:.0f} frames/s", file=sys.stderr)
    t_get, t_enq, t_slot, t_rel = waits
    # start-up (imports, ctx, tables, pinning the slots) and the exit are outside this figure; the first read and the last write are inside it
    print(f"staging: pipeline {index} frames in {t_pipe:.3f} s = {index / max(t_pipe, 1e-9):.0f} frames/s (first read issued ... last batch written)", file=sys.stderr)
    print(f"staging: start-up imports {t_imports:.3f} s, device + ctx + tables {t_engine:.3f} s, files + staging slots {t_slots:.3f} s", file=sys.stderr)
    print(f"staging: input {reader.mapped_batches} batches mapped (hipHostRegister {reader.rmap.t_reg if reader.rmap else 0.0:.3f}s), {reader.staged_batches} staged"
          f"{' — ' + reader.note if reader.note else ''} | output {writer.mapped_batches} batches mapped (register + page allocation {writer.t_prep:.3f}s)"
          f"{' — ' + writer.note if writer.note else ''} | pipe buffers in {pipes[0]} out {pipes[1]} bytes", file=sys.stderr)
    print(f"staging: reader read {reader.t_io:.3f}s waited-for-slot {reader.t_wait:.3f}s | feeder waited-for-input {t_get:.3f}s enqueued {t_enq:.3f}s "
          f"waited-for-output-slot {t_slot:.3f}s waited-for-upload {t_rel:.3f}s | writer waited-for-download {writer.t_wait:.3f}s wrote {writer.t_io:.3f}s",
          file=sys.stderr)


def main(argv=None) -> int:
    a = add_input_flags(add_output_flags(build_parser())).parse_args(argv)
    spec, ranks = check_flags(a)
    if ranks is not None:
        return main_sharded(a, spec, *ranks)
    t_start = time.perf_counter()
    import torch
    from .pipeline import FramePipeline
    from .staging import _Reader, _Writer
    from .text import make_text_overlay_rgba
    t_imports = time.perf_counter() - t_start
    rs = settings_from_args(a)
    fps_out = int(a.fps) if a.fps and a.fps > 0 else 24            # ref:914
    h, w = int(a.height), int(a.width)
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device visible; pythoncrt_amd has no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device())
    seed = a.noise_seed if a.noise_seed is not None else int.from_bytes(os.urandom(8), "little")
    overlay = make_text_overlay_rgba(w, h, a.text, a.text_font, a.text_size, a.text_color, (a.text_x, a.text_y)) if a.text else None   # ref:1076
    pix = torch.float16 if spec.half else torch.uint8              # 10-bit formats on both ends, or --chain-pix half: the chain runs on half pixels
    pipe = FramePipeline(dev, h, w, rs, fps=fps_out, noise_seed=seed, dtype=pix, text_overlay_rgba=overlay, text_overlay_after=bool(a.text_after))
    t_engine = time.perf_counter() - t_start - t_imports
    fin = sys.stdin.buffer if a.input == "-" else open(a.input, "rb", buffering=0)
    out_path = a.output if a.output else (a.input + "_crt.rgb" if a.input != "-" else "-")
    NS, ratio = 3, spec.ratio                                      # delivery frames per input frame
    B, Bs = spec.batch(a.batch)                                    # the chain's batch, input frames per batch
    end = spec.delivery_end(dev, pix)
    source = None if spec.direct else spec.source_end(dev, (h, w), pix)      # every stage in front of the chain gives an rgb24 input a source end too
    in_bytes = h * w * 3 if source is None else source.frame_bytes
    t0 = time.perf_counter()
    fout, in_pos, out_pos, pipes, out_plan = open_output(a, fin, out_path, B, in_bytes, end.frame_bytes, ratio, end.frames)
    jobs = ((k * Bs * in_bytes if in_pos else None, Bs) for k in itertools.count())     # whole batches until the stream ends (the reader stops at a short read)
    reader = _Reader(fin, in_pos, jobs, (B, h, w, 3) if source is None else (Bs,) + source.frame_shape, in_bytes, slots=NS, io=a.io, autostart=False)
    writer = _Writer(fout, out_pos, end.shape(end.frames(B)), end.frame_bytes, slots=NS, plan=out_plan, io=a.io)
    t_pipe = time.perf_counter()                                    # the pipeline proper: first read issued ... last batch written (the --staging-report line)
    t_slots = t_pipe - t_start - t_imports - t_engine
    index, marks, waits = feed(pipe, source, end, reader, writer, NS, fout if out_pos else None, a.staging_report)
    t_pipe = time.perf_counter() - t_pipe
    reader.close()
    fout.flush()
    if out_pos:
        os.ftruncate(fout.fileno(), index * end.frame_bytes)  # an input that ended before its planned length, an output file that was longer
    if fout is not sys.stdout.buffer:
        fout.close()
    if fin is not sys.stdin.buffer:
        fin.close()
    print(f"{index} frames, elapsed {time.perf_counter() - t0:.3f}s", file=sys.stderr)      # ref:1269
    if a.staging_report:
        staging_report(index, marks, waits, (t_pipe, t_imports, t_engine, t_slots), reader, writer, pipes)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
