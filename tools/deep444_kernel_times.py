"""Dev tool (GPU box): what the 10-bit 4:4:4 source and egress kernels (include/crtfx_444.h) cost per frame — both directions, both
layouts, vec and general path, 1080p and 4K — next to the yardstick of this box: a device-to-device copy of the same traffic per frame in
the same batches.  A planar frame (6 bytes per pixel) and its half RGB frame (6) are 12 * h * w bytes of traffic, an x2rgb10le frame (4)
and its half RGB frame 10 * h * w; a copy moves every byte twice, so the yardsticks copy 6 * h * w and 5 * h * w bytes per frame.

    python tools/deep444_kernel_times.py run [--no-clock]      # HIP-event times per frame, the copy yardsticks, the shader clock while it ran

Per size / direction / layout / path it launches WARM + a per-size number of batches of FRAMES frames on one stream between two events, so
that every timed window lasts 0.1 s or more (8000 batches at 1080p, 2000 at 4K); the rows of one size are taken ROUNDS times in turn (the
two copies, then every kernel build) so that a drift of the clock shows as spread between the rounds, and the median per row is printed
beside the smallest and largest.  It measures throughput against the copy of equal traffic, nothing else."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [("1080p", 1080, 1920, 8000), ("4K", 2160, 3840, 2000)]      # name, h, w, timed batches per row and round: windows of 0.1 s and more
FRAMES, WARM, ROUNDS = 8, 3, 3
LAYOUTS = (("planar", "yuv444p10le", 6), ("x2rgb10le", "x2rgb10le", 5))     # token of last_plan, a format of that layout, copy bytes per pixel


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
    from pythoncrt_amd import _lib
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
        copies = {}                                             # layout token -> (source, destination) of the yardstick copy
        for token, _, per_px in LAYOUTS:
            a = torch.randint(0, 256, (FRAMES, per_px * h * w), dtype=torch.uint8, device=dev)
            copies[token] = (a, torch.empty_like(a))
        rgb = (torch.randint(0, 1021, (FRAMES, h, w, 3), dtype=torch.int16, device=dev).to(torch.float16) / 4)      # quarter codes
        rows, keep = [], []                                     # (label, layout token, callable, bytes moved per frame)
        for kind, cls, opt in (("unpack444", pc.UnpackDeep444, _lib.UNPACK444_OPT_FORCE_GENERAL), ("egress444", pc.EgressDeep444, _lib.EGRESS444_OPT_FORCE_GENERAL)):
            for token, fmt, _ in LAYOUTS:
                for force in (False, True):
                    plan = cls(dev, (h, w), layout=fmt)
                    plan.set_option(opt, int(force))
                    packed = torch.randint(0, 256, (FRAMES, plan.frame_bytes), dtype=torch.uint8, device=dev)
                    src, out = (packed, torch.empty_like(rgb)) if kind == "unpack444" else (rgb, torch.empty_like(packed))
                    plan.run(src, out=out)
                    rows.append((plan.plan()[kind], token, (lambda p=plan, s=src, o=out: p.run(s, out=o)), 6 * h * w + plan.frame_bytes))
                    keep.append((plan, packed, out))
        copy_us, times = {t: [] for t in copies}, [[] for _ in rows]
        for _ in range(ROUNDS):
            for t, (a, b) in copies.items():
                copy_us[t].append(_timed(lambda a=a, b=b: b.copy_(a), runs))
            for i, (_, _, fn, _) in enumerate(rows):
                times[i].append(_timed(fn, runs))
        cmed = {t: statistics.median(v) for t, v in copy_us.items()}
        for token, _, per_px in LAYOUTS:
            nbytes, v = per_px * h * w, copy_us[token]
            print(f"{name:6s} device-to-device copy of {per_px}*h*w = {nbytes / 1e6:.2f} MB per frame ({token}): {cmed[token]:8.1f} ({min(v):.1f} .. {max(v):.1f}) us/frame = "
                  f"{2 * nbytes / cmed[token] / 1e3:6.0f} GB/s read + write", flush=True)
        for (label, token, _, moved), t in zip(rows, times):
            med = statistics.median(t)
            print(f"{name:6s} {label:36s} {med:8.1f} ({min(t):.1f} .. {max(t):.1f}) us/frame = {moved / med / 1e3:6.0f} GB/s of {moved / 1e6:.1f} MB in + out; "
                  f"{med / cmed[token]:5.2f} x the copy", flush=True)
        for plan, _, _ in keep:
            plan.close()
        del copies, rgb, rows, keep
    if tel is not None:
        print(f"shader clock / power while it ran: {tel.stop()}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        run(clock="--no-clock" not in sys.argv)
        sys.exit(0)
    print(__doc__)
    sys.exit(2)
