"""Dev tool (GPU box): what the 10-bit source and egress kernels (include/crtfx_deep.h) cost per frame — both directions, both layouts, vec
and general path, 1080p, 4K and 8K — next to the yardstick of this box: a device-to-device copy of 4.5 * h * w bytes per frame in the same
batches (a copy moves every byte twice: the same 9 bytes per pixel of traffic as 3 of 4:2:0 words on one side and 6 of half RGB on the
other).  And the two ends of the pipeline with 8-bit and with 10-bit 4:2:0 frames.

    python tools/deep_kernel_times.py run                      # HIP-event times per frame, the copy yardstick, the shader clock while it ran
    python tools/deep_kernel_times.py e2e [--repeats R]        # process_frames and the CLI at 4K: rgb24 and nv12 (uint8 chain) against p010le (half chain)
    rocprofv3 --kernel-trace --stats -d DIR -o deep --output-format csv -- python tools/deep_kernel_times.py run --no-clock

`run` launches, per size / direction / layout / path, WARM + RUNS batches of FRAMES frames on one stream between two events.  It measures
throughput against the copy of equal traffic, nothing else."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [("1080p", 1080, 1920), ("4K", 2160, 3840), ("8K", 4320, 7680)]
FRAMES, WARM, RUNS = 4, 3, 30


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
    return e0.elapsed_time(e1) * 1e3 / (RUNS * FRAMES)          # us per frame, launch gaps included


def run(clock=True):
    import torch
    import pythoncrt_amd as pc
    from pythoncrt_amd import _lib
    dev = torch.device("cuda", torch.cuda.current_device())
    tel = None
    if clock:
        import bench
        tel = bench.GpuTelemetry(dev)
        tel.start()
    print(f"device: {torch.cuda.get_device_name(dev)}; batches of {FRAMES} frames, {WARM} warm-up + {RUNS} timed batches per row, HIP events on one stream", flush=True)
    for name, h, w in SIZES:
        nbytes = int(4.5 * h * w)
        a = torch.randint(0, 256, (FRAMES, nbytes), dtype=torch.uint8, device=dev)
        b = torch.empty_like(a)
        copy_us = _timed(lambda: b.copy_(a))
        print(f"{name:6s} device-to-device copy of 4.5*h*w = {nbytes / 1e6:.2f} MB per frame: {copy_us:8.1f} us/frame = {2 * nbytes / copy_us / 1e3:6.0f} GB/s read + write",
              flush=True)
        del a, b
        packed = torch.randint(0, 256, (FRAMES, pc.deep.frame_bytes(h, w)), dtype=torch.uint8, device=dev)       # any words: the stages ignore the spare bits
        rgb = (torch.rand((FRAMES, h, w, 3), device=dev) * 255.0).to(torch.float16)
        for kind, cls, opt in (("unpack10", pc.UnpackYuv10, _lib.UNPACK10_OPT_FORCE_GENERAL), ("egress10", pc.EgressYuv10, _lib.EGRESS10_OPT_FORCE_GENERAL)):
            for layout in ("yuv420p10le", "p010le"):
                for force in (0, 1):
                    plan = cls(dev, (h, w), layout=layout)
                    plan.set_option(opt, force)
                    src, out = (packed, torch.empty_like(rgb)) if kind == "unpack10" else (rgb, torch.empty_like(packed))
                    us = _timed(lambda: plan.run(src, out=out))
                    moved = 6 * h * w + plan.frame_bytes
                    print(f"{name:6s} {plan.plan()[kind]:40s} {us:8.1f} us/frame = {moved / us / 1e3:6.0f} GB/s of {moved / 1e6:.1f} MB in + out; "
                          f"{us / copy_us:5.2f} x the copy", flush=True)
                    plan.close()
                    del out
        del packed, rgb
    if tel is not None:
        print(f"shader clock / power while it ran: {tel.stop()}", flush=True)


# (label, process_frames keywords, CLI flags, input file, bytes per pixel written)
E2E = [("rgb24 in,  rgb24 out       (uint8 chain)", {}, [], "rgb", 3.0),
       ("nv12 in,   nv12 out        (uint8 chain)", {"in_pix_fmt": "nv12", "out_pix_fmt": "nv12"}, ["--in-pix-fmt", "nv12", "--out-pix-fmt", "nv12"], "nv12", 1.5),
       ("p010le in, yuv420p10le out (half chain) ", {"in_pix_fmt": "p010le", "out_pix_fmt": "yuv420p10le"},
        ["--in-pix-fmt", "p010le", "--out-pix-fmt", "yuv420p10le"], "p010", 3.0)]


def e2e(repeats=3):
    """process_frames (in-memory iterator, a writer that does nothing) and the CLI (file to file on the temporary directory, --io staged) at
    4K with the reference CLI's default settings: frames/s per input / output format, `repeats` runs each."""
    import subprocess
    import tempfile
    import numpy as np
    import pythoncrt_amd as pc
    h, w, n = 2160, 3840, 64
    rng = np.random.default_rng(0)
    frames = {"rgb": [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(8)],
              "nv12": [rng.integers(0, 256, h * w * 3 // 2, dtype=np.uint8) for _ in range(8)],
              "p010": [(rng.integers(0, 1024, h * w * 3 // 2).astype(np.uint16) << 6).view(np.uint8) for _ in range(8)]}
    for label, kw, _, key, _ in E2E:
        base = frames[key]
        pc.process_frames(iter(base), lambda a: None, w, h, 30, 8, noise_seed=1, **kw)
        rates = []
        for _ in range(repeats):
            t = time.perf_counter()
            k = pc.process_frames((base[i % 8] for i in range(n)), lambda a: None, w, h, 30, n, noise_seed=1, **kw)
            rates.append(k / (time.perf_counter() - t))
        print(f"process_frames 4K {label}: " + ", ".join(f"{r:.0f}" for r in rates) + f" frames/s ({n} frames per run, set-up of the call included)", flush=True)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory(dir=os.environ.get("CRTFX_TMP") or None) as tmp:
        for key, base in frames.items():
            with open(os.path.join(tmp, "in." + key), "wb") as f:
                for i in range(n):
                    f.write(base[i % 8].tobytes())
        for label, _, flags, key, bpp_out in E2E:
            src = os.path.join(tmp, "in." + key)
            rates = []
            for _ in range(repeats + 1):                         # the first run warms the page cache and is dropped
                cmd = [sys.executable, "-m", "pythoncrt_amd.cli", "--input", src, "--output", os.path.join(tmp, "out.raw"), "--width", str(w), "--height", str(h),
                       "--fps", "30", "--noise-seed", "1", "--staging-report"] + flags
                r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    print(r.stderr[-2000:], file=sys.stderr)
                    return 2
                line = [ln for ln in r.stderr.splitlines() if "staging: pipeline" in ln][-1]
                rates.append(float(line.split(" = ")[1].split()[0]))
                size = os.path.getsize(os.path.join(tmp, "out.raw"))
                assert size == int(n * h * w * bpp_out), size
            print(f"CLI 4K file -> file {label}: " + ", ".join(f"{r:.0f}" for r in rates[1:]) + f" frames/s (first read issued ... last batch written; {n} frames, "
                  f"input {os.path.getsize(src) / n / 1e6:.1f} MB, output {size / n / 1e6:.1f} MB per frame)", flush=True)
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        run(clock="--no-clock" not in sys.argv)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "e2e":
        sys.exit(e2e(int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 3))
    print(__doc__)
    sys.exit(2)
