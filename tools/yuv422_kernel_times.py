"""Dev tool (GPU box): what the 8-bit 4:2:2 source and egress kernels (include/crtfx_422.h) cost per frame — both directions, all three
layouts, vec and general path, 1080p and 4K — next to the yardstick of this box: a device-to-device copy of 2.5 * h * w bytes per frame in
the same batches (a copy moves every byte twice: the same 5 bytes per pixel of traffic as 2 of 4:2:2 on one side and 3 of rgb24 on the
other).

    python tools/yuv422_kernel_times.py run [--no-clock]       # HIP-event times per frame, the copy yardstick, the shader clock while it ran

Per size / direction / layout / path it launches WARM + a per-size number of batches of FRAMES frames on one stream between two events, so
that every timed window lasts 0.1 s or more (8000 batches at 1080p, 2000 at 4K); the rows of one
size are taken ROUNDS times in turn (copy, then every kernel build) so that a drift of the clock shows as spread between the rounds, and
the median per row is printed beside the smallest and largest.  It measures throughput against the copy of equal traffic, nothing else."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [("1080p", 1080, 1920, 8000), ("4K", 2160, 3840, 2000)]      # name, h, w, timed batches per row and round: windows of 0.1 s and more
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
    from pythoncrt_amd import yuv422
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device visible: nothing is measured without one")
    dev = torch.device("cuda", torch.cuda.current_device())
    tel = None
    if clock:
        import bench
        tel = bench.GpuTelemetry(dev)
        tel.start()
    print(f"device: {torch.cuda.get_device_name(dev)}; batches of {FRAMES} frames, {WARM} warm-up + "
          f"{' / '.join(str(s[3]) for s in SIZES)} ({' / '.join(s[0] for s in SIZES)}) timed batches per row and round, {ROUNDS} rounds, HIP events on one stream; median (min .. max) of the rounds", flush=True)
    for name, h, w, runs in SIZES:
        nbytes = int(2.5 * h * w)
        a = torch.randint(0, 256, (FRAMES, nbytes), dtype=torch.uint8, device=dev)
        b = torch.empty_like(a)
        rgb = torch.randint(0, 256, (FRAMES, h, w, 3), dtype=torch.uint8, device=dev)
        rows = []                                               # (label, callable, bytes moved per frame)
        keep = []
        for kind, cls in (("unpack422", pc.UnpackYuv422), ("egress422", pc.EgressYuv422)):
            for layout in ("yuv422p", "yuyv422", "uyvy422"):
                for force in (False, True):
                    plan = cls(dev, (h, w), layout, force_general=force)
                    packed = torch.randint(0, 256, (FRAMES, yuv422.frame_bytes(h, w, layout)), dtype=torch.uint8, device=dev)
                    src, out = (packed, torch.empty_like(rgb)) if kind == "unpack422" else (rgb, torch.empty_like(packed))
                    plan(src, out=out)
                    rows.append((plan.plan()[kind], (lambda p=plan, s=src, o=out: p(s, out=o)), 3 * h * w + plan.frame_bytes))
                    keep.append((plan, packed, out))
        copy_us, times = [], [[] for _ in rows]
        for _ in range(ROUNDS):
            copy_us.append(_timed(lambda: b.copy_(a), runs))
            for i, (_, fn, _) in enumerate(rows):
                times[i].append(_timed(fn, runs))
        cmed = statistics.median(copy_us)
        print(f"{name:6s} device-to-device copy of 2.5*h*w = {nbytes / 1e6:.2f} MB per frame: {cmed:8.1f} ({min(copy_us):.1f} .. {max(copy_us):.1f}) us/frame = "
              f"{2 * nbytes / cmed / 1e3:6.0f} GB/s read + write", flush=True)
        for (label, _, moved), t in zip(rows, times):
            med = statistics.median(t)
            print(f"{name:6s} {label:32s} {med:8.1f} ({min(t):.1f} .. {max(t):.1f}) us/frame = {moved / med / 1e3:6.0f} GB/s of {moved / 1e6:.1f} MB in + out; "
                  f"{med / cmed:5.2f} x the copy", flush=True)
        for plan, _, _ in keep:
            plan.close()
        del a, b, rgb, rows, keep
    if tel is not None:
        print(f"shader clock / power while it ran: {tel.stop()}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        run(clock="--no-clock" not in sys.argv)
        sys.exit(0)
    print(__doc__)
    sys.exit(2)
