"""Dev tool (GPU box): what the sited egress kernels (include/crtfx_egress_sited.h) cost per frame — every layout, vec and general path,
siting left and center, 1080p and 4K — next to two yardsticks taken in the same run: the BOX egress stage of the same format (EgressYuv /
EgressYuv422 / EgressYuv10, both paths), and a device-to-device copy of the same traffic per frame in the same batches.  An RGB frame and
its frame of frame_bytes are rgb_bytes + frame_bytes of traffic (4.5 * h * w for 8-bit 4:2:0, 5 for 4:2:2, 9 for 10-bit 4:2:0); a copy
moves every byte twice, so the yardsticks copy half of that per frame.

    python tools/egress_sited_kernel_times.py run [--no-clock]      # HIP-event times per frame, the yardsticks, the shader clock while it ran

Per size and row it launches WARM + a per-size number of batches of FRAMES frames on one stream between two events, so that every timed
window lasts about 0.1 s or more; the rows of one size are taken ROUNDS times in turn (the copies, then every kernel build) so that a drift
of the clock shows as spread between the rounds, and the median per row is printed beside the smallest and largest.  It measures throughput
against the box stage and the copy of equal traffic, nothing else.  A summary line per size and layout closes the table: the vec build
at siting left against the box stage's vec build, the copy and its own general build."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [("1080p", 1080, 1920, 4000), ("4K", 2160, 3840, 1000)]      # name, h, w, timed batches per row and round
FRAMES, WARM, ROUNDS = 8, 3, 3


def _timed(fn, runs):
    import torch
    for _ in range(WARM):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(runs):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (runs * FRAMES)          # us per frame, launch gaps included


def run(clock=True):
    import torch
    import pythoncrt_amd as pc
    from pythoncrt_amd import formats, sited
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device visible: nothing is measured without one")
    dev = torch.device("cuda", torch.cuda.current_device())
    tel = None
    if clock:
        import bench
        tel = bench.GpuTelemetry(dev)
        tel.start()
    print(f"device: {torch.cuda.get_device_name(dev)}; batches of {FRAMES} frames, {WARM} warm-up + "
          f"{' / '.join(str(s[3]) for s in SIZES)} ({' / '.join(s[0] for s in SIZES)}) timed batches per row and round, {ROUNDS} rounds, HIP events on one stream; "
          "median (min .. max) of the rounds", flush=True)
    for name, h, w, runs in SIZES:
        rows, keep, copies = [], [], {}                         # (label, traffic, callable); traffic in bytes per frame -> (a, b) of its copy
        for layout in sited.LAYOUTS:
            deep = formats.bits(layout) == 10
            fb = sited.frame_bytes(h, w, layout)
            moved = fb + h * w * (6 if deep else 3)
            if moved not in copies:
                a = torch.randint(0, 256, (FRAMES, moved // 2), dtype=torch.uint8, device=dev)
                copies[moved] = (a, torch.empty_like(a))
            if deep:                                            # halves on the 0..255 scale, eighths: the quantiser rounds
                frames = (torch.randint(0, 2048, (FRAMES, h, w, 3), device=dev).to(torch.float32) / 8.0).to(torch.float16)
            else:
                frames = torch.randint(0, 256, (FRAMES, h, w, 3), dtype=torch.uint8, device=dev)
            out = torch.empty((FRAMES, fb), dtype=torch.uint8, device=dev)
            keep.append((frames, out))
            plans = [(formats.FORMATS[layout].egress(dev, (h, w), layout=layout), force, None) for force in (False, True)]
            plans += [(pc.EgressSited(dev, (h, w), layout, siting=siting), force, siting) for force in (False, True) for siting in ("left", "center")]
            for plan, force, siting in plans:
                plan.force_general = force
                plan.run(frames, out=out)
                key = next(k for k in plan.plan() if k not in ("frames", "siting"))
                label = plan.plan()[key] + (f" {siting}" if siting else " (box)")
                rows.append((label, moved, (lambda p=plan, s=frames, o=out: p.run(s, out=o)), layout, siting, force))
                keep.append(plan)
        copy_us, times = {m: [] for m in copies}, [[] for _ in rows]
        for _ in range(ROUNDS):
            for m, (a, b) in copies.items():
                copy_us[m].append(_timed(lambda a=a, b=b: b.copy_(a), runs))
            for i, row in enumerate(rows):
                times[i].append(_timed(row[2], runs))
        cmed = {m: statistics.median(v) for m, v in copy_us.items()}
        for m, v in copy_us.items():
            print(f"{name:6s} device-to-device copy of {m / 2 / (h * w):.2f}*h*w = {m / 2e6:.2f} MB per frame: {cmed[m]:8.1f} ({min(v):.1f} .. {max(v):.1f}) us/frame = "
                  f"{m / cmed[m] / 1e3:6.0f} GB/s read + write", flush=True)
        med = [statistics.median(t) for t in times]
        base = {(row[3], row[5]): med[i] for i, row in enumerate(rows) if row[4] is None}      # the box build of the same layout and path
        for (label, moved, _, layout, siting, force), t, m in zip(rows, times, med):
            print(f"{name:6s} {label:52s} {m:8.1f} ({min(t):.1f} .. {max(t):.1f}) us/frame = {moved / m / 1e3:6.0f} GB/s of {moved / 1e6:.1f} MB in + out; "
                  f"{m / cmed[moved]:5.2f} x the copy" + (f"; {m / base[(layout, force)]:5.2f} x the box build" if siting else ""), flush=True)
        mine = {(row[3], row[4], row[5]): med[i] for i, row in enumerate(rows) if row[4] is not None}
        for layout in sited.LAYOUTS:
            moved = next(row[1] for row in rows if row[3] == layout)
            v, g = mine[(layout, "left", False)], mine[(layout, "left", True)]
            print(f"{name:6s} summary {layout:12s} vec left {v:7.1f} us/frame = {v / base[(layout, False)]:5.2f} x the box vec build, {v / cmed[moved]:5.2f} x the copy; "
                  f"general {g:7.1f} = {g / v:5.2f} x vec; vec center {mine[(layout, 'center', False)]:7.1f}", flush=True)
        for item in keep:
            if hasattr(item, "close"):
                item.close()
        del copies, rows, keep
    if tel is not None:
        print(f"shader clock / power while it ran: {tel.stop()}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        run(clock="--no-clock" not in sys.argv)
        sys.exit(0)
    print(__doc__)
    sys.exit(2)
