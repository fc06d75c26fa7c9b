"""Dev tool (GPU box): what the geometry stage (include/crtfx_canvas.h) costs per frame, uint8 and half, vec path and general path, for the
pads and crops a user of process_frames(deliver_fit=, in_crop=) meets, next to a yardstick measured in the same run: a device-to-device
copy of the same traffic (the window's bytes read + the canvas's bytes written).

    python tools/canvas_kernel_times.py run                      # HIP-event times per frame (launch gaps included) + the copies + ratios
    rocprofv3 --kernel-trace --stats -d DIR -o canvas --output-format csv -- python tools/canvas_kernel_times.py run
    python tools/canvas_kernel_times.py report DIR               # kernel time per frame from the trace

`run` launches, per case and sample type, ROUNDS rounds of (vec, general, copy), each WARM + RUNS batches of FRAMES frames timed with HIP
events over the RUNS back-to-back batches, and prints the best round of each (the rounds alternate so that a neighbour's load on the
machine hits all three) and the ratios to the copy.  The copy is torch's `copy_` of a buffer of half the traffic (it is read and written).
`report` walks the trace's k_canvas dispatches in that order, drops each WARM part, and prints mean kernel time per frame."""
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name, source size, destination size, window (y, x, h, w) or None = the whole source, placement (dst_y, dst_x)
CASES = [("pad 2160x2880 -> 2160x3840 dx=480", (2160, 2880), (2160, 3840), None, (0, 480)),
         ("pad 1080x1440 -> 1080x1920 dx=240", (1080, 1440), (1080, 1920), None, (0, 240)),
         ("pad 1080x1440 -> 1080x1920 dx=241", (1080, 1440), (1080, 1920), None, (0, 241)),
         ("crop 1600x3840 at y=280 of 2160x3840", (2160, 3840), (1600, 3840), (280, 0, 1600, 3840), (0, 0)),
         ("crop 2160x2880 at x=481 of 2160x3840", (2160, 3840), (2160, 2880), (0, 481, 2160, 2880), (0, 0))]
FRAMES, WARM, RUNS, ROUNDS = 8, 3, 20, 3


def moved_bytes(src, dst, window, itemsize):
    wh, ww = (window[2], window[3]) if window else src
    return 3 * itemsize * (wh * ww + dst[0] * dst[1])


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
    dev = torch.device("cuda", torch.cuda.current_device())
    print(f"batches of {FRAMES} frames, {WARM} warm-up + {RUNS} timed batches per figure, best of {ROUNDS} alternating rounds; us per frame from HIP "
          "events (launch gaps included); traffic = window bytes read + canvas bytes written", flush=True)
    for name, src, dst, window, at in CASES:
        for what, dtype in (("uint8", torch.uint8), ("half", torch.float16)):
            frames = torch.randint(0, 256, (FRAMES,) + src + (3,), dtype=torch.uint8, device=dev).to(dtype)
            out = torch.empty((FRAMES,) + dst + (3,), dtype=dtype, device=dev)
            mb = moved_bytes(src, dst, window, frames.element_size())
            a = torch.empty((FRAMES, mb // 2), dtype=torch.uint8, device=dev)
            b = torch.empty_like(a)
            plans = [pc.Canvas(dev, src, dst, window=window, at=at, fill=(16, 128, 128), dtype=dtype, force_general=force) for force in (False, True)]
            best = {}
            for _ in range(ROUNDS):
                for key, fn in (("vec", lambda: plans[0].run(frames, out=out)), ("general", lambda: plans[1].run(frames, out=out)),
                                ("copy", lambda: b.copy_(a))):
                    us = _timed(fn)
                    best[key] = min(us, best.get(key, us))
            assert plans[0].plan()["canvas"].endswith(",vec>") and plans[1].plan()["canvas"].endswith(",general>")
            for key, label in (("vec", plans[0].plan()["canvas"]), ("general", plans[1].plan()["canvas"]), ("copy", "device-to-device copy of equal traffic")):
                print(f"{name:38s} {what:5s} {label:40s} {best[key]:8.1f} us/frame {mb / best[key] / 1e3:6.0f} GB/s of {mb / 1e6:5.1f} MB"
                      + ("" if key == "copy" else f"   {best[key] / best['copy']:5.2f} x the copy"), flush=True)
            for p in plans:
                p.close()
            del frames, out, a, b
            torch.cuda.synchronize()


def report(directory):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        print(f"no *kernel_trace.csv under {directory}", file=sys.stderr)
        return 2
    rows = []
    for f in files:
        for row in csv.DictReader(open(f)):
            if "k_canvas" in row["Kernel_Name"]:
                rows.append((int(row["Start_Timestamp"]), "general" if "general" in row["Kernel_Name"] else "vec",
                             int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    rows.sort()
    pos = 0
    for name, src, dst, window, at in CASES:
        for what, itemsize in (("uint8", 1), ("half", 2)):
            times = {"vec": [], "general": []}
            for _ in range(ROUNDS):
                for path in ("vec", "general"):
                    for batch in range(WARM + RUNS):
                        if pos >= len(rows) or rows[pos][1] != path:
                            print(f"trace does not follow the run's order at dispatch {pos}: expected {path}", file=sys.stderr)
                            return 2
                        if batch >= WARM:
                            times[path].append(rows[pos][2])
                        pos += 1
            mb = moved_bytes(src, dst, window, itemsize)
            for path, v in times.items():
                us = sum(v) / len(v) / 1e3 / FRAMES
                print(f"{name:38s} {what:5s} {path:8s} {us:8.1f} us/frame {mb / us / 1e3:6.0f} GB/s of {mb / 1e6:5.1f} MB   "
                      f"({len(v)} dispatches of {FRAMES} frames, min {min(v) / 1e3 / FRAMES:.1f}, max {max(v) / 1e3 / FRAMES:.1f})")
    if pos != len(rows):
        print(f"{len(rows) - pos} canvas dispatches beyond the run's sequence", file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "report":
        sys.exit(report(sys.argv[2]))
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        run()
        sys.exit(0)
    print(__doc__)
    sys.exit(2)
