"""Dev tool (GPU box): what the PAL composite-video stage (include/crtfx_pal.h) costs per frame — uint8 / half x composite / svideo x sharp /
soft x delay / simple x vec path / general path; 576 x 720 and 1080 x 1920 — next to two yardsticks measured in the same run: the
untouched k_signal<same signal, chroma, pix, vec> (include/crtfx_signal.h: the same row cascade without the strip, the rotation and the
delay line) and a device-to-device copy of the same traffic (one frame read, one written).

    python tools/pal_kernel_times.py run                        # HIP-event times per frame (launch gaps included) + the yardsticks + ratios

`run` launches, per size and kind, ROUNDS rounds of (vec, general, k_signal, copy), each WARM + RUNS batches of FRAMES frames timed with
HIP events over the RUNS back-to-back batches, and prints the best round of each (the rounds alternate so that a neighbour's load on the
machine hits all four) and the ratios to k_signal, to the copy and between the paths.  The copy is torch's `copy_` of a buffer of one
frame's bytes per frame (it is read and written).  The library under test is the one pythoncrt_amd loads (CRTFX_LIB names another build,
e.g. one compiled with -DCRTFX_PAL_STRIP=16); the first line of the output names it."""
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [("576", (576, 720)), ("1080", (1080, 1920))]
PIXES = ["u8", "f16"]
FRAMES, WARM, RUNS, ROUNDS = 8, 3, 20, 3


def moved_bytes(size, pix):
    """Of one frame: it is read once (the halo between segments and the strip's extra row are a few per cent and lie in the cache) and written once."""
    return size[0] * size[1] * 3 * (2 if pix == "f16" else 1) * 2


def _timed(fn):
    import torch
    for _ in range(WARM):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(RUNS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (RUNS * FRAMES)


def run(label=""):
    import torch
    import pythoncrt_amd as pc
    from pythoncrt_amd import _lib
    from pythoncrt_amd.pal import DECODERS
    from pythoncrt_amd.signal import CHROMAS, SIGNALS
    dev = torch.device("cuda", torch.cuda.current_device())
    print(f"library {os.path.relpath(_lib.LIB_PATH, _lib.ROOT)} {label}".rstrip())
    print(f"batches of {FRAMES} frames, {WARM} warm-up + {RUNS} timed batches per figure, best of {ROUNDS} alternating rounds; us per frame from "
          "HIP events (launch gaps included); traffic = one frame read + one frame written", flush=True)
    for (name, size), pix in itertools.product(SIZES, PIXES):
        mb = moved_bytes(size, pix)
        if pix == "u8":
            frames = torch.randint(0, 256, (FRAMES,) + size + (3,), dtype=torch.uint8, device=dev)
        else:
            frames = torch.randint(0, 1021, (FRAMES,) + size + (3,), dtype=torch.int16, device=dev).to(torch.float16) / 4
        out = torch.empty_like(frames)
        a = torch.empty((FRAMES, mb // 2), dtype=torch.uint8, device=dev)
        b = torch.empty_like(a)
        for signal, chroma in itertools.product(SIGNALS, CHROMAS):
            ntsc = pc.Signal(dev, size, signal=signal, chroma=chroma, dtype=frames.dtype)
            for decoder in DECODERS:
                plans = [pc.PalSignal(dev, size, signal=signal, chroma=chroma, decoder=decoder, phase=20, dtype=frames.dtype, force_general=force)
                         for force in (False, True)]
                best = {}
                for _ in range(ROUNDS):
                    for key, fn in (("vec", lambda: plans[0].run(frames, out=out)), ("general", lambda: plans[1].run(frames, out=out)),
                                    ("ntsc", lambda: ntsc.run(frames, out=out)), ("copy", lambda: b.copy_(a))):
                        us = _timed(fn)
                        best[key] = min(us, best.get(key, us))
                assert plans[0].plan()["pal"].endswith("vec>") and plans[1].plan()["pal"].endswith("general>")
                assert ntsc.plan()["signal"].endswith("vec>")
                for key, label_ in (("vec", plans[0].plan()["pal"]), ("general", plans[1].plan()["pal"]), ("ntsc", ntsc.plan()["signal"]),
                                    ("copy", "device-to-device copy of equal traffic")):
                    print(f"{name:5s} {label_:46s} {best[key]:8.2f} us/frame {mb / best[key] / 1e3:6.0f} GB/s of {mb / 1e6:5.1f} MB"
                          + ("" if key in ("copy", "ntsc") else f"   {best[key] / best['ntsc']:6.2f} x k_signal   {best[key] / best['copy']:6.2f} x the copy")
                          + (f"   {best['general'] / best['vec']:5.2f} x the vec path" if key == "general" else ""), flush=True)
                for p in plans:
                    p.close()
            ntsc.close()
        del frames, out, a, b
        torch.cuda.synchronize()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        run(" ".join(sys.argv[2:]))
        sys.exit(0)
    print(__doc__)
    sys.exit(2)
