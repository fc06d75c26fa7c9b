"""Dev tool (GPU box): what the field-paired 4:2:0 egress kernels (include/crtfx_egress_field420.h) cost per frame — every layout, vec and
general path, chroma center and left, 480 x 720, 1080 x 1920 and 4K — next to two yardsticks taken in the same run: the untouched
k_egress_sited<layout,vec> at siting left (EgressSited: the same bytes out, one RGB read where this stage has up to two), and a
device-to-device copy of the same traffic per frame in the same batches.  An RGB frame and its frame of frame_bytes are rgb_bytes +
frame_bytes of traffic (4.5 * h * w for 8-bit, 9 for 10-bit); a copy moves every byte twice, so the yardstick copies half of that per frame.

    python tools/egress_field420_kernel_times.py run [--no-clock]   # HIP-event times per frame, the yardsticks, the shader clock while it ran
    python tools/egress_field420_kernel_times.py run --frames 64 --only 480p      # one size in larger batches: 480 x 720 in batches of 8 is
                                                                                  # bound by the launches, not by the kernels

Per size and row it launches WARM + a per-size number of batches of FRAMES frames on one stream between two events, so that every timed
window lasts about 0.1 s or more; the rows of one size are taken ROUNDS times in turn (the copies, then every kernel build) so that a drift
of the clock shows as spread between the rounds, and the median per row is printed beside the smallest and largest.  It measures throughput
against the sited stage and the copy of equal traffic, nothing else.  A summary line per size and layout closes the table: the vec build
at chroma left against the sited vec build, the copy, its own general build and its own centre run."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [("480p", 480, 720, 4000), ("1080p", 1080, 1920, 3000), ("4K", 2160, 3840, 1000)]      # name, h, w, timed batches per row and round
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


def run(clock=True, per_batch=None, only=None):
    global FRAMES
    import torch
    import pythoncrt_amd as pc
    from pythoncrt_amd import field420, formats
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device visible: nothing is measured without one")
    dev = torch.device("cuda", torch.cuda.current_device())
    if per_batch:                                               # the same number of frames per timed window
        sizes = [(n, h, w, max(1, runs * FRAMES // per_batch)) for n, h, w, runs in SIZES if only in (None, n)]
        FRAMES = per_batch
    else:
        sizes = [s for s in SIZES if only in (None, s[0])]
    tel = None
    if clock:
        import bench
        tel = bench.GpuTelemetry(dev)
        tel.start()
    print(f"device: {torch.cuda.get_device_name(dev)}; batches of {FRAMES} frames, {WARM} warm-up + "
          f"{' / '.join(str(s[3]) for s in sizes)} ({' / '.join(s[0] for s in sizes)}) timed batches per row and round, {ROUNDS} rounds, HIP events on one stream; "
          "median (min .. max) of the rounds", flush=True)
    for name, h, w, runs in sizes:
        rows, keep, copies = [], [], {}                         # (label, traffic, callable, ...); traffic in bytes per frame -> (a, b) of its copy
        for layout in field420.LAYOUTS:
            deep = formats.bits(layout) == 10
            fb = field420.frame_bytes(h, w, layout)
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
            plans = [(pc.EgressSited(dev, (h, w), layout, siting="left"), False, None)]
            plans += [(pc.EgressField420(dev, (h, w), layout, chroma=chroma), force, chroma) for force in (False, True) for chroma in ("left", "center")]
            for plan, force, chroma in plans:
                plan.force_general = force
                plan.run(frames, out=out)
                key = next(k for k in plan.plan() if k not in ("frames", "siting", "chroma"))
                label = plan.plan()[key] + (f" {chroma}" if chroma else " left (sited)")
                rows.append((label, moved, (lambda p=plan, s=frames, o=out: p.run(s, out=o)), layout, chroma, force))
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
        base = {row[3]: med[i] for i, row in enumerate(rows) if row[4] is None}                # the sited vec build of the same layout
        for (label, moved, _, layout, chroma, force), t, m in zip(rows, times, med):
            print(f"{name:6s} {label:56s} {m:8.2f} ({min(t):.2f} .. {max(t):.2f}) us/frame = {moved / m / 1e3:6.0f} GB/s of {moved / 1e6:.1f} MB in + out; "
                  f"{m / cmed[moved]:5.2f} x the copy" + (f"; {m / base[layout]:5.2f} x the sited vec build" if chroma else ""), flush=True)
        mine = {(row[3], row[4], row[5]): med[i] for i, row in enumerate(rows) if row[4] is not None}
        for layout in field420.LAYOUTS:
            moved = next(row[1] for row in rows if row[3] == layout)
            v, g = mine[(layout, "left", False)], mine[(layout, "left", True)]
            print(f"{name:6s} summary {layout:12s} vec left {v:7.2f} us/frame = {v / base[layout]:5.2f} x the sited vec build, {v / cmed[moved]:5.2f} x the copy; "
                  f"general {g:7.2f} = {g / v:5.2f} x vec; vec center {mine[(layout, 'center', False)]:7.2f}; general center {mine[(layout, 'center', True)]:7.2f}", flush=True)
        for item in keep:
            if hasattr(item, "close"):
                item.close()
        del copies, rows, keep
    if tel is not None:
        print(f"shader clock / power while it ran: {tel.stop()}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        opt = {k: sys.argv[sys.argv.index(k) + 1] for k in ("--frames", "--only") if k in sys.argv}
        run(clock="--no-clock" not in sys.argv, per_batch=int(opt.get("--frames", 0)), only=opt.get("--only"))
        sys.exit(0)
    print(__doc__)
    sys.exit(2)
