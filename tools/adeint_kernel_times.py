"""Dev tool (GPU box): what the motion-adaptive deinterlace stage (include/crtfx_adeint.h) costs per SOURCE frame — uint8 / half x first /
both x vec path / general path; 480 x 720 and 1080 x 1920 — next to two yardsticks measured in the same run: a device-to-device copy of
the same traffic (each source frame read once + the output frames written) and the untouched k_deint<edge,...> builds of
include/crtfx_deint.h, the spatial method it falls back to.

    python tools/adeint_kernel_times.py run                     # HIP-event times per frame (launch gaps included) + the yardsticks + ratios

`run` launches, per size and kind, ROUNDS rounds of (vec, general, EDGE vec, EDGE general, copy), each WARM + RUNS batches of FRAMES
source frames timed with HIP events over the RUNS back-to-back batches, and prints the best round of each (the rounds alternate so that a
neighbour's load on the machine hits all five) and the ratios to the copy and to EDGE on the same path.  Every source frame has a
previous frame (frame 0 the caller's), and each frame is the one before it with half its rows redrawn, so both sides of the rule run.
The copy is torch's `copy_` of a buffer of half the traffic (it is read and written)."""
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [("480i", (480, 720)), ("1080i", (1080, 1920))]
PIXES = ["u8", "f16"]
FRAMES, WARM, RUNS, ROUNDS = 8, 3, 20, 3


def moved_bytes(size, pix, fields):
    """Of one source frame: it is read once (as C, and again from the caches as the next frame's P), and one or two frames are written."""
    return size[0] * size[1] * 3 * (2 if pix == "f16" else 1) * (1 + (2 if fields == "both" else 1))


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
    from pythoncrt_amd.deint import FIELDS
    dev = torch.device("cuda", torch.cuda.current_device())
    print(f"batches of {FRAMES} source frames, {WARM} warm-up + {RUNS} timed batches per figure, best of {ROUNDS} alternating rounds; us per SOURCE "
          "frame from HIP events (launch gaps included); traffic = each source frame read once + the output frames written", flush=True)
    for (name, size), pix, fields in itertools.product(SIZES, PIXES, FIELDS):
        mb = moved_bytes(size, pix, fields)
        per = 2 if fields == "both" else 1
        if pix == "u8":
            frames = torch.randint(0, 256, (FRAMES + 1,) + size + (3,), dtype=torch.uint8, device=dev)
        else:
            frames = torch.randint(0, 1021, (FRAMES + 1,) + size + (3,), dtype=torch.int16, device=dev).to(torch.float16) / 4
        still = torch.rand(size[0], device=dev) < 0.5
        for i in range(1, FRAMES + 1):                       # half the rows of every frame are those of the frame before it
            frames[i, still] = frames[i - 1, still]
        prev, frames = frames[0], frames[1:]
        out = torch.empty((FRAMES * per,) + size + (3,), dtype=frames.dtype, device=dev)
        a = torch.empty((FRAMES, mb // 2), dtype=torch.uint8, device=dev)
        b = torch.empty_like(a)
        plans = [pc.AdaptiveDeinterlace(dev, size, order="tff", fields=fields, dtype=frames.dtype, force_general=force) for force in (False, True)]
        edges = [pc.Deinterlace(dev, size, method="edge", order="tff", fields=fields, dtype=frames.dtype, force_general=force) for force in (False, True)]
        best = {}
        for _ in range(ROUNDS):
            for key, fn in (("vec", lambda: plans[0].run(frames, out=out, prev=prev)), ("general", lambda: plans[1].run(frames, out=out, prev=prev)),
                            ("edge vec", lambda: edges[0].run(frames, out=out)), ("edge general", lambda: edges[1].run(frames, out=out)),
                            ("copy", lambda: b.copy_(a))):
                us = _timed(fn)
                best[key] = min(us, best.get(key, us))
        assert plans[0].plan()["adeint"].endswith("vec>") and plans[1].plan()["adeint"].endswith("general>")
        assert edges[0].plan()["deint"].endswith("vec>") and edges[1].plan()["deint"].endswith("general>")
        for key, label in (("vec", plans[0].plan()["adeint"]), ("general", plans[1].plan()["adeint"]), ("edge vec", edges[0].plan()["deint"]),
                           ("edge general", edges[1].plan()["deint"]), ("copy", "device-to-device copy of equal traffic")):
            ratios = "" if key == "copy" else f"   {best[key] / best['copy']:5.2f} x the copy"
            if key in ("vec", "general"):
                ratios += f"   {best[key] / best['edge ' + key]:5.2f} x EDGE"
            print(f"{name:6s} {label:40s} {best[key]:8.1f} us/frame {mb / best[key] / 1e3:6.0f} GB/s of {mb / 1e6:5.1f} MB" + ratios, flush=True)
        print(f"{name:6s} {pix} {fields}: vec / general = {best['vec'] / best['general']:.2f}", flush=True)
        for p in plans + edges:
            p.close()
        del frames, prev, out, a, b
        torch.cuda.synchronize()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        run()
        sys.exit(0)
    print(__doc__)
    sys.exit(2)
