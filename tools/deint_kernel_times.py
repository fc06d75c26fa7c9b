"""Dev tool (GPU box): what the deinterlace stage (include/crtfx_deint.h) costs per SOURCE frame — uint8 / half x linear / edge x first /
both x vec path / general path; 480 x 720 and 1080 x 1920 — next to a yardstick measured in the same run: a device-to-device copy of the
same traffic (one source frame read + the output frames written).

    python tools/deint_kernel_times.py run                      # HIP-event times per frame (launch gaps included) + the copies + ratios

`run` launches, per size and kind, ROUNDS rounds of (vec, general, copy), each WARM + RUNS batches of FRAMES source frames timed with HIP
events over the RUNS back-to-back batches, and prints the best round of each (the rounds alternate so that a neighbour's load on the
machine hits all three) and the ratios to the copy.  The copy is torch's `copy_` of a buffer of half the traffic (it is read and
written)."""
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [("480i", (480, 720)), ("1080i", (1080, 1920))]
PIXES = ["u8", "f16"]
FRAMES, WARM, RUNS, ROUNDS = 8, 3, 20, 3


def moved_bytes(size, pix, fields):
    """Of one source frame: it is read once, and one or two frames of its size are written."""
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
    from pythoncrt_amd.deint import FIELDS, METHODS
    dev = torch.device("cuda", torch.cuda.current_device())
    print(f"batches of {FRAMES} source frames, {WARM} warm-up + {RUNS} timed batches per figure, best of {ROUNDS} alternating rounds; us per SOURCE "
          "frame from HIP events (launch gaps included); traffic = one source frame read + the output frames written", flush=True)
    for (name, size), pix, method, fields in itertools.product(SIZES, PIXES, METHODS, FIELDS):
        mb = moved_bytes(size, pix, fields)
        per = 2 if fields == "both" else 1
        if pix == "u8":
            frames = torch.randint(0, 256, (FRAMES,) + size + (3,), dtype=torch.uint8, device=dev)
        else:
            frames = torch.randint(0, 1021, (FRAMES,) + size + (3,), dtype=torch.int16, device=dev).to(torch.float16) / 4
        out = torch.empty((FRAMES * per,) + size + (3,), dtype=frames.dtype, device=dev)
        a = torch.empty((FRAMES, mb // 2), dtype=torch.uint8, device=dev)
        b = torch.empty_like(a)
        plans = [pc.Deinterlace(dev, size, method=method, order="tff", fields=fields, dtype=frames.dtype, force_general=force) for force in (False, True)]
        best = {}
        for _ in range(ROUNDS):
            for key, fn in (("vec", lambda: plans[0].run(frames, out=out)), ("general", lambda: plans[1].run(frames, out=out)),
                            ("copy", lambda: b.copy_(a))):
                us = _timed(fn)
                best[key] = min(us, best.get(key, us))
        assert plans[0].plan()["deint"].endswith("vec>") and plans[1].plan()["deint"].endswith("general>")
        for key, label in (("vec", plans[0].plan()["deint"]), ("general", plans[1].plan()["deint"]), ("copy", "device-to-device copy of equal traffic")):
            print(f"{name:6s} {label:40s} {best[key]:8.1f} us/frame {mb / best[key] / 1e3:6.0f} GB/s of {mb / 1e6:5.1f} MB"
                  + ("" if key == "copy" else f"   {best[key] / best['copy']:5.2f} x the copy"), flush=True)
        for p in plans:
            p.close()
        del frames, out, a, b
        torch.cuda.synchronize()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        run()
        sys.exit(0)
    print(__doc__)
    sys.exit(2)
