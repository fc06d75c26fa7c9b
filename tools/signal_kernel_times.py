"""Dev tool (GPU box): what the composite-video stage (include/crtfx_signal.h) costs per frame — uint8 / half x composite / svideo x sharp /
soft x vec path / general path; 480 x 720 and 1080 x 1920 — next to two yardsticks measured in the same run: a device-to-device copy of
the same traffic (one frame read, one written), and the untouched k_deint<edge,pix,first,vec> (one frame read, one written as well).

    python tools/signal_kernel_times.py run                     # HIP-event times per frame (launch gaps included) + the yardsticks + ratios

`run` launches, per size and kind, ROUNDS rounds of (vec, general, copy, deint), each WARM + RUNS batches of FRAMES frames timed with HIP
events over the RUNS back-to-back batches, and prints the best round of each (the rounds alternate so that a neighbour's load on the
machine hits all four) and the ratios to the copy and between the paths.  The copy is torch's `copy_` of a buffer of one frame's bytes per
frame (it is read and written)."""
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [("480", (480, 720)), ("1080", (1080, 1920))]
PIXES = ["u8", "f16"]
FRAMES, WARM, RUNS, ROUNDS = 8, 3, 20, 3


def moved_bytes(size, pix):
    """Of one frame: it is read once (the halo between segments is a few per cent and lies in the cache) and written once."""
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


def run():
    import torch
    import pythoncrt_amd as pc
    from pythoncrt_amd.signal import CHROMAS, SIGNALS
    dev = torch.device("cuda", torch.cuda.current_device())
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
        deint = pc.Deinterlace(dev, size, method="edge", order="tff", fields="first", dtype=frames.dtype)
        for signal, chroma in itertools.product(SIGNALS, CHROMAS):
            plans = [pc.Signal(dev, size, signal=signal, chroma=chroma, dtype=frames.dtype, force_general=force) for force in (False, True)]
            best = {}
            for _ in range(ROUNDS):
                for key, fn in (("vec", lambda: plans[0].run(frames, out=out)), ("general", lambda: plans[1].run(frames, out=out)),
                                ("copy", lambda: b.copy_(a)), ("deint", lambda: deint.run(frames, out=out))):
                    us = _timed(fn)
                    best[key] = min(us, best.get(key, us))
            assert plans[0].plan()["signal"].endswith("vec>") and plans[1].plan()["signal"].endswith("general>")
            assert deint.plan()["deint"].endswith("first,vec>")
            for key, label in (("vec", plans[0].plan()["signal"]), ("general", plans[1].plan()["signal"]),
                               ("copy", "device-to-device copy of equal traffic"), ("deint", deint.plan()["deint"])):
                print(f"{name:5s} {label:46s} {best[key]:8.2f} us/frame {mb / best[key] / 1e3:6.0f} GB/s of {mb / 1e6:5.1f} MB"
                      + ("" if key in ("copy", "deint") else f"   {best[key] / best['copy']:6.2f} x the copy")
                      + (f"   {best['general'] / best['vec']:5.2f} x the vec path" if key == "general" else ""), flush=True)
            for p in plans:
                p.close()
        deint.close()
        del frames, out, a, b
        torch.cuda.synchronize()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        run()
        sys.exit(0)
    print(__doc__)
    sys.exit(2)
