"""Dev tool (GPU box): frames/s of pythoncrt_amd.process_frames fed by an in-memory iterator of numpy frames and a writer that does nothing — the
ceiling of the Python-level drop-in for process_video's loop (ref:1037-1131), host side included (one memcpy per frame into the pinned batch,
PCIe both ways, the per-frame write_frame call).

    python tools/process_frames_rate.py                                           # 1080p and 4K, source at the output size, both settings
    python tools/process_frames_rate.py --size 2160x3840 --source 1080x1920       # a 1080p source rendered at 4K (resized on the device)
    python tools/process_frames_rate.py --size 2160x3840 --source 1080x1920 --resize-on host --frames 48     # ... by Pillow on the host
    python tools/process_frames_rate.py --size 2160x3840 --out-pix-fmt yuv420p --deliver 1080x1920            # a 4K render delivered as 1080p yuv420p
    python tools/process_frames_rate.py --size 2160x2880 --out-pix-fmt yuv420p --deliver 1080x1920 --deliver-fit pad  # a 4:3 render pillarboxed in 1080p
    options: --frames N (per repeat), --repeats R, --chain full|default|both, --out-pix-fmt FMT, --deliver HxW (process_frames(deliver_size=)),
             --deliver-fit stretch|pad|crop (process_frames(deliver_fit=))"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pythoncrt_amd as pc

CHAINS = {"default": ("reference CLI defaults", {}),
          "full": ("full chain: Gaussian bloom sigma 3 + warp 0.15", dict(fast_bloom=False, bloom_sigma=3.0, warp_strength=0.15, pixel_size=1, persistence=0.0))}


def hw(text):
    h, w = text.lower().split("x")
    return int(h), int(w)


def opt(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


size, source, resize_on = opt("--size"), opt("--source"), opt("--resize-on")
sizes = [hw(size) + (int(opt("--frames", 160)),)] if size else [(1080, 1920, int(opt("--frames", 480))), (2160, 3840, int(opt("--frames", 160)))]
chains = [CHAINS[c] for c in (("default", "full") if opt("--chain", "both") == "both" else (opt("--chain"),))]
extra = {"resize_on": resize_on} if resize_on else {}          # absent: the package's default
if opt("--out-pix-fmt"):
    extra["out_pix_fmt"] = opt("--out-pix-fmt")
if opt("--deliver"):
    extra["deliver_size"] = hw(opt("--deliver"))
if opt("--deliver-fit"):
    extra["deliver_fit"] = opt("--deliver-fit")
for (h, w, n) in sizes:
    sh, sw = hw(source) if source else (h, w)
    rng = np.random.default_rng(0)
    base = [rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8) for _ in range(8)]
    for name, kw in chains:
        pc.process_frames(iter(base), lambda a: None, w, h, 30, 8, noise_seed=1, **kw, **extra)                 # warm-up: ctx, tables, pinned slots
        for _ in range(int(opt("--repeats", 1))):
            t = time.perf_counter()
            k = pc.process_frames((base[i % 8] for i in range(n)), lambda a: None, w, h, 30, n, noise_seed=1, **kw, **extra)
            dt = time.perf_counter() - t
            src = "" if (sh, sw) == (h, w) else f" from a {sw}x{sh} source (resize_on={resize_on or 'default'})"
            if "deliver_size" in extra or "out_pix_fmt" in extra:
                dh, dw = extra.get("deliver_size", (h, w))
                src += f" written as {dw}x{dh} {extra.get('out_pix_fmt', 'rgb24')}" + (f" (deliver_fit={extra['deliver_fit']})" if "deliver_fit" in extra else "")
            print(f"{w}x{h}{src} {name}: {k} frames in {dt:.3f} s = {k / dt:.0f} frames/s (set-up of the call included)", flush=True)
