"""Host I/O staging of the CLI: the reader and writer threads, their pinned slots, the file I/O behind them and the registered mappings of
`--io mapped`.  What each path is for is told in `cli.__doc__` ("Host staging", "Regular files skip the pinned staging ...")."""
from __future__ import annotations

import time

import numpy as np


def _read_into(fin, view: memoryview) -> int:
    """Fill `view` from a file or pipe; returns the bytes read (short only at end of stream)."""
    got = 0
    while got < len(view):
        k = fin.readinto(view[got:])
        if not k:
            break
        got += k
    return got


_IO_POOL = None
_IO_SLICE = 8 << 20             # bytes per positional read / write / copy call


def _io_pool():
    """Threads for positional file I/O: one os.preadv / os.pwrite moves ~8 GB/s out of / into the page cache (a memcpy on one core,
    GIL released), a 4K frame is 24.9 MB each way — the raw rgb24 edge, not the GPU, would set the CLI's frame rate."""
    global _IO_POOL
    if _IO_POOL is None:
        import concurrent.futures
        import os
        try:
            cpus = len(os.sched_getaffinity(0))
        except (AttributeError, OSError):
            cpus = os.cpu_count() or 2
        want = int(os.environ.get("CRTFX_IO_THREADS", "0") or 0)          # A/B knob (tools/cli_throughput.sh); default: half the cpus, at most 16
        _IO_POOL = concurrent.futures.ThreadPoolExecutor(max_workers=want if want > 0 else max(1, min(16, cpus // 2)), thread_name_prefix="crtfx-io")
    return _IO_POOL


def _pread_full(fd: int, view: memoryview, offset: int) -> int:
    """Fill `view` from `fd` at `offset` (regular file) in parallel slices; returns the bytes read (short only at end of file)."""
    import os

    def one(lo):
        hi, got = min(len(view), lo + _IO_SLICE), 0
        while lo + got < hi:
            k = os.preadv(fd, [view[lo + got:hi]], offset + lo + got)
            if k <= 0:
                break
            got += k
        return got
    starts = range(0, len(view), _IO_SLICE)
    parts = list(_io_pool().map(one, starts)) if len(view) > _IO_SLICE else [one(0)]
    total = 0
    for lo, got in zip(starts, parts):          # contiguous prefix actually read
        total += got
        if got < min(len(view), lo + _IO_SLICE) - lo:
            break
    return total


_LIBC = None


def _madvise(addr: int, length: int, advice: int) -> int:
    """madvise(2) through ctypes: the call runs WITHOUT the GIL (mmap.madvise of CPython 3.10 keeps it), so the zapper thread's drops of a
    400 MB batch (~13 ms) never hold up the Python threads that feed the GPU."""
    global _LIBC
    if _LIBC is None:
        import ctypes
        _LIBC = ctypes.CDLL(None, use_errno=True)
        _LIBC.madvise.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        _LIBC.madvise.restype = ctypes.c_int
    return _LIBC.madvise(addr, length, advice)


class _MappedInput:
    """A regular input file mapped read-only: a batch is copied out of the page cache by user-space memcpy on the I/O threads
    (numpy's copy loop releases the GIL) instead of read(2).  Measured on the GPU box, 1.6 GB from tmpfs into a pinned buffer, eight
    threads (tools/io_rates.py): 76 GB/s — against 18 GB/s for os.preadv on the FIRST read of a freshly written file (61 GB/s on later
    reads), which is what capped the CLI at ~700 4K frames/s whatever the GPU side did.  MADV_WILLNEED on the batch after next starts
    the readahead of a file that is not in the page cache yet."""

    def __init__(self, fd: int):
        import mmap
        import os
        self.fd, self._os = fd, os
        self.size = os.fstat(fd).st_size
        self.map = mmap.mmap(fd, self.size, prot=mmap.PROT_READ) if self.size > 0 else None
        self.arr = np.frombuffer(self.map, dtype=np.uint8) if self.map is not None else None
        self.base = int(self.arr.ctypes.data) if self.arr is not None else 0
        self._mmap = mmap
        # the page-table entries of what has been copied are dropped (the pages stay in the page cache) by ONE thread of its own, batch by
        # batch behind the copies: unmapping costs ~0.15 us per 4 KB page wherever it is paid — in one piece at exit 0.9 s for a 24 GB clip;
        # from the sixteen copy threads, slice by slice, the drops contend in the kernel (tmpfs: 28 ms per 400 MB batch when they really run in
        # parallel, 17 ms serialised by the GIL as in round 4) and sit on the reader's critical path; one thread beside the copies does
        # a batch in ~13 ms and delays nobody (profiles/r05_cli_throughput.txt)
        import queue
        import threading
        self._zap_q = queue.Queue()
        self._zap_mode = os.environ.get("CRTFX_IO_DONTNEED", "thread")      # A/B knob: "thread" (default) | "0" (never: left to process exit) | "slice" (on the copy threads, round 4)
        self._zap_thr = None
        self._zap_err = False
        if self.map is not None and self._zap_mode == "thread" and hasattr(mmap, "MADV_DONTNEED"):
            def zapper():
                while True:
                    job = self._zap_q.get()
                    if job is None:
                        return
                    a0, a1 = job
                    while a0 < a1 and not self._zap_err:
                        k = min(a1 - a0, 32 << 20)
                        if _madvise(self.base + a0, k, mmap.MADV_DONTNEED) != 0:
                            self._zap_err = True      # the first failure ends the drops (they are an optimisation): a raw address is never advised blindly
                        a0 += k
            self._zap_thr = threading.Thread(target=zapper, name="crtfx-zap", daemon=True)
            self._zap_thr.start()

    def read_into(self, dst: np.ndarray, offset: int) -> int:
        """Fill the uint8 array `dst` from the file at `offset`; returns the bytes copied (short only at end of file)."""
        # a file that was truncated under us ends the clip early (a short read, as read(2) would report it) instead of a SIGBUS from the
        # pages that are gone: the size is looked at again before every batch
        try:
            now = self._os.fstat(self.fd).st_size
        except OSError:
            now = self.size
        n = max(0, min(dst.size, min(self.size, now) - offset))
        if n <= 0:
            return 0
        ahead = min(self.size, offset + 3 * dst.size) - (offset + n)
        if ahead > 0 and hasattr(self._mmap, "MADV_WILLNEED"):
            page = self._mmap.PAGESIZE
            lo = ((offset + n) // page) * page
            _madvise(self.base + lo, min(self.size - lo, ahead + page), self._mmap.MADV_WILLNEED)

        page = self._mmap.PAGESIZE
        drop = getattr(self._mmap, "MADV_DONTNEED", None) if self._zap_mode == "slice" else None

        def one(lo):
            hi = min(n, lo + _IO_SLICE)
            np.copyto(dst[lo:hi], self.arr[offset + lo:offset + hi])
            # CRTFX_IO_DONTNEED=slice (round 4's form, kept for the A/B): drop the page-table entries of what this thread has copied, slice by
            # slice on the I/O threads; the default hands the whole batch to the zapper thread below instead
            if drop is not None:
                a0, a1 = ((offset + lo + page - 1) // page) * page, ((offset + hi) // page) * page
                if a1 > a0:
                    try:
                        self.map.madvise(drop, a0, a1 - a0)      # mmap.madvise keeps the GIL: the drops of the sixteen threads run one after the other (on purpose, see __init__)
                    except (OSError, ValueError):
                        pass
        if n > _IO_SLICE:
            list(_io_pool().map(one, range(0, n, _IO_SLICE)))
        else:
            one(0)
        if self._zap_thr is not None:
            a0, a1 = ((offset + page - 1) // page) * page, ((offset + n) // page) * page
            if a1 > a0:
                self._zap_q.put((a0, a1))
        return n

    def close(self):
        if self._zap_thr is not None:
            self._zap_q.put(None)
            self._zap_thr.join()                    # no timeout: the thread advises RAW addresses of this mapping, which must outlive it (a drop of a
            self._zap_thr = None                    # 400 MB batch takes ~13 ms; the queue holds at most the batches read)
        self.arr = None
        if self.map is not None:
            try:
                self.map.close()
            except BufferError:         # a view of the map is still referenced somewhere: the mapping goes with the process
                pass
            self.map = None


def _pwrite_full(fd: int, view: memoryview, offset: int) -> None:
    """Write `view` to `fd` at `offset` (regular file) in parallel slices."""
    import os

    def one(lo):
        hi, pos = min(len(view), lo + _IO_SLICE), lo
        while pos < hi:                              # os.pwrite may write less than asked
            k = os.pwrite(fd, view[pos:hi], offset + pos)
            if k <= 0:
                raise SystemExit(f"short write at byte {offset + pos}")
            pos += k
    if len(view) > _IO_SLICE:
        list(_io_pool().map(one, range(0, len(view), _IO_SLICE)))
    elif len(view):
        one(0)


def _seekable(f) -> bool:
    import os
    import stat
    try:
        return stat.S_ISREG(os.fstat(f.fileno()).st_mode)
    except (OSError, ValueError, AttributeError):
        return False


def _grow_pipe(f, want: int = 0) -> int:
    """F_SETPIPE_SZ on a pipe end (Linux): the default 64 KiB buffer makes a 24.9 MB 4K frame 380 wake-ups of the process on the other
    side; 1 MiB is what an unprivileged process may ask for (/proc/sys/fs/pipe-max-size).  Returns the buffer size now in force (0: not a
    pipe / not supported)."""
    import fcntl
    import os
    import stat
    try:
        fd = f.fileno()
        if not stat.S_ISFIFO(os.fstat(fd).st_mode):
            return 0
        if want <= 0:                              # CRTFX_PIPE_SIZE: A/B of the buffer size (tools/cli_throughput.sh); 0 bytes = leave the pipe as it is
            want = int(os.environ.get("CRTFX_PIPE_SIZE", 1 << 20))
        F_SETPIPE_SZ, F_GETPIPE_SZ = getattr(fcntl, "F_SETPIPE_SZ", 1031), getattr(fcntl, "F_GETPIPE_SZ", 1032)
        try:
            if want > 0:
                fcntl.fcntl(fd, F_SETPIPE_SZ, want)
        except OSError:
            pass                                   # above pipe-max-size: keep what we have
        return int(fcntl.fcntl(fd, F_GETPIPE_SZ))
    except (OSError, ValueError, AttributeError):
        return 0


class _HostDma:
    """hipHostRegister / hipHostUnregister / hipMemcpyAsync of the HIP runtime this process has already loaded (torch's), through ctypes —
    plain pointers and sizes.  What they are for: the PCIe DMA engines read a batch straight out of, or write it straight into, a shared
    mapping of the raw rgb24 FILE (the page cache), with no pinned staging copy on the host."""
    H2D, D2H = 1, 2
    _lib = None

    @classmethod
    def lib(cls):
        if cls._lib is None:
            import ctypes
            path = None
            try:
                with open("/proc/self/maps") as maps:
                    for line in maps:
                        if "libamdhip64" in line:
                            path = line.split()[-1]
                            break
            except OSError:
                pass
            lib = ctypes.CDLL(path or "libamdhip64.so")
            lib.hipHostRegister.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint]
            lib.hipHostRegister.restype = ctypes.c_int
            lib.hipHostUnregister.argtypes = [ctypes.c_void_p]
            lib.hipHostUnregister.restype = ctypes.c_int
            lib.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
            lib.hipMemcpyAsync.restype = ctypes.c_int
            lib.hipGetLastError.restype = ctypes.c_int
            cls._lib = lib
        return cls._lib

    @classmethod
    def register(cls, ptr: int, n: int) -> bool:
        lib = cls.lib()
        if lib.hipHostRegister(ptr, n, 0) != 0:
            lib.hipGetLastError()                  # clear the sticky error: the caller falls back to staging
            return False
        return True

    @classmethod
    def unregister(cls, ptr: int):
        if cls.lib().hipHostUnregister(ptr) != 0:
            cls.lib().hipGetLastError()

    @classmethod
    def copy(cls, dst: int, src: int, n: int, kind: int, stream: int):
        rc = cls.lib().hipMemcpyAsync(dst, src, n, kind, stream)
        if rc != 0:
            raise RuntimeError(f"hipMemcpyAsync failed with error {rc}")


_MAPPED_MIN_GBS = 30.0          # --io auto: registration slower than this per byte (tmpfs: 13-17 GB/s) loses to the memcpy staging


class _RegisteredMap:
    """A MAP_SHARED mapping of a regular file whose pages the GPU's DMA engines address directly.  Windows of WIN bytes (page multiples,
    on a fixed grid so that the page two neighbouring batches share is never registered twice) are registered with the HIP runtime when a
    batch first needs them and unregistered when the last batch using them is done."""
    WIN = 32 << 20

    def __init__(self, fd: int, size: int, writable: bool):
        import mmap
        import threading
        self.size = int(size)
        self.map = mmap.mmap(fd, self.size, flags=mmap.MAP_SHARED, prot=mmap.PROT_READ | (mmap.PROT_WRITE if writable else 0))
        self.arr = np.frombuffer(self.map, dtype=np.uint8)
        self.base = int(self.arr.ctypes.data)
        self.maplen = -(-self.size // mmap.PAGESIZE) * mmap.PAGESIZE
        self.ref, self.lock = {}, threading.Lock()
        self.t_reg = 0.0                        # seconds spent in hipHostRegister

    def _span(self, w):
        lo = w * self.WIN
        return lo, min(self.WIN, self.maplen - lo)

    def acquire(self, off: int, n: int) -> bool:
        """Make the bytes [off, off + n) DMA-addressable; False when the runtime refuses (nothing stays registered for this call)."""
        ws = range(off // self.WIN, (off + n - 1) // self.WIN + 1)
        done = []
        with self.lock:
            for w in ws:
                if self.ref.get(w, 0) == 0:
                    lo, ln = self._span(w)
                    t = time.perf_counter()
                    ok = _HostDma.register(self.base + lo, ln)
                    self.t_reg += time.perf_counter() - t
                    if not ok:
                        for v in done:
                            self._drop(v)
                        return False
                self.ref[w] = self.ref.get(w, 0) + 1
                done.append(w)
        return True

    def _drop(self, w):
        c = self.ref.get(w, 0) - 1
        if c <= 0:
            self.ref.pop(w, None)
            _HostDma.unregister(self.base + w * self.WIN)
        else:
            self.ref[w] = c

    def release(self, off: int, n: int):
        with self.lock:
            for w in range(off // self.WIN, (off + n - 1) // self.WIN + 1):
                self._drop(w)

    def copy(self, kind: int, dev_ptr: int, off: int, n: int, stream: int):
        """hipMemcpyAsync between device memory at dev_ptr and the file bytes [off, off + n), window by window: every window is a
        registration of its own, and the runtime rejects a single copy that runs across two of them."""
        pos = 0
        while pos < n:
            w = (off + pos) // self.WIN
            k = min(n - pos, (w + 1) * self.WIN - (off + pos))
            host = self.base + off + pos
            if kind == _HostDma.H2D:
                _HostDma.copy(dev_ptr + pos, host, k, kind, stream)
            else:
                _HostDma.copy(host, dev_ptr + pos, k, kind, stream)
            pos += k

    def close(self):
        with self.lock:
            for w in list(self.ref):
                _HostDma.unregister(self.base + w * self.WIN)
            self.ref.clear()
        self.arr = None
        try:
            self.map.close()
        except (BufferError, ValueError):
            pass


class _MapTok:
    """One batch that lives in a registered file mapping: byte range + the flow-control slot it holds."""
    __slots__ = ("off", "nbytes", "slot")

    def __init__(self, off, nbytes, slot):
        self.off, self.nbytes, self.slot = off, nbytes, slot


class _PinnedSlots:
    """The pinned uint8 slots of `_Reader` and `_Writer`, each pinned when first asked for (the mapped paths may never need one)."""

    def __init__(self, shape, slots: int):
        import threading
        import torch
        self._torch, self.shape = torch, shape
        self._bufs = [None] * slots
        self._pin_lock = threading.Lock()

    def _buf(self, i):
        if self._bufs[i] is None:
            with self._pin_lock:
                if self._bufs[i] is None:
                    self._bufs[i] = self._torch.empty(self.shape, dtype=self._torch.uint8).pin_memory()
        return self._bufs[i]

    @property
    def bufs(self):
        return [self._buf(i) for i in range(len(self._bufs))]


class _Reader(_PinnedSlots):
    """A thread that gets input batches ready ahead of the GPU.  `jobs` yields (byte offset | None, frames) requests — an offset for
    positional reads of a regular file, None for the next bytes of a stream — and `get()` hands back (token, frames, bytes) in order, or
    None at the end; `upload(token, frames, dst, stream)` enqueues the batch's host-to-device copy and `release(token)` returns its slot
    once that copy has completed.  Two ways a batch gets ready:
      staged   filled into a pinned (B, H, W, 3) uint8 slot (token = slot index): read(2) / readinto for a stream, memcpy out of a
               private mapping on the I/O threads for a regular file;
      mapped   (io = "mapped" / "auto", regular files) the windows of a SHARED mapping of the file that the batch covers are registered
               with the HIP runtime and the upload reads the page cache itself (token = _MapTok).  "auto" times the first batch and goes
               back to staging when registration is refused or runs below _MAPPED_MIN_GBS."""

    def __init__(self, fin, positional: bool, jobs, shape, frame_bytes: int, slots: int = 3, io: str = "staged", autostart: bool = True):
        import os
        import queue
        import threading
        super().__init__(shape, slots)
        self.fin, self.positional, self.frame_bytes = fin, positional, frame_bytes
        self.free, self.full = queue.Queue(), queue.Queue()      # the free-slot queue already bounds what is in flight
        for i in range(slots):
            self.free.put(i)
        self.err = None
        self.t_wait = self.t_io = 0.0          # seconds this thread waited for a free slot / spent reading (the --staging-report line)
        self.mapped = None                     # private mapping the staged path copies out of
        self.rmap = None                       # shared, registered mapping of the mapped path
        self.mode = "staged"                   # what the NEXT batch will use
        self.mapped_batches = self.staged_batches = 0
        self.note = ""
        if positional:
            try:
                self.mapped = _MappedInput(fin.fileno())
                if self.mapped.map is None:
                    self.mapped = None
            except (OSError, ValueError):
                self.mapped = None             # not mappable: positional read(2) calls instead
            if io in ("mapped", "auto") and self.mapped is not None:
                try:
                    self.rmap = _RegisteredMap(fin.fileno(), self.mapped.size, writable=False)
                    self.mode = "mapped"
                except (OSError, ValueError, AttributeError) as e:
                    self.note = f"input mapping refused ({e.__class__.__name__}): staged"
        if self.mode == "staged":
            # pinned up front, as the GPU loop expects when it starts.  (Six 16-frame 4K slots take 0.5 s of hipHostMalloc; pinning all but the
            # first on a helper thread beside the first batches was tried in round 5: the pipeline then ran 0.25 s longer — the runtime
            # serialises the allocations with the copies' enqueues — and the run as a whole no shorter.)
            for i in range(slots):
                self._buf(i)

        def stage(i, off, nfr):
            view = memoryview(self._buf(i).numpy()).cast("B")[: nfr * frame_bytes]
            if self.mapped is not None:
                got = self.mapped.read_into(self._buf(i).numpy().reshape(-1)[: nfr * frame_bytes], off)
            else:
                got = _pread_full(fin.fileno(), view, off) if positional else _read_into(fin, view)
            self.staged_batches += 1
            return i, got, len(view)

        def map_batch(i, off, nfr):
            """-> (token, got, wanted) or None when this batch has to be staged"""
            try:
                now = os.fstat(fin.fileno()).st_size
            except OSError:
                now = self.rmap.size
            want = nfr * frame_bytes
            got = max(0, min(want, min(self.rmap.size, now) - off))
            nbytes = (got // frame_bytes) * frame_bytes
            if nbytes:
                t = time.perf_counter()
                ok = self.rmap.acquire(off, nbytes)
                dt = time.perf_counter() - t
                if not ok:
                    self.mode, self.note = "staged", "hipHostRegister refused the input mapping: staged"
                    return None
                if io == "auto" and self.mapped_batches == 0 and nbytes / max(dt, 1e-9) / 1e9 < _MAPPED_MIN_GBS:
                    # this batch is registered and is used as it is; the ones behind it are staged
                    self.mode = "staged"
                    self.note = f"registering the input mapping ran at {nbytes / max(dt, 1e-9) / 1e9:.1f} GB/s (< {_MAPPED_MIN_GBS:.0f}): staged from the second batch on"
            self.mapped_batches += 1
            return _MapTok(off, nbytes, i), got, want

        def loop():
            try:
                for off, nfr in jobs:
                    t = time.perf_counter()
                    i = self.free.get()
                    self.t_wait += time.perf_counter() - t
                    if i is None:
                        return
                    t = time.perf_counter()
                    res = map_batch(i, off, nfr) if self.mode == "mapped" else None
                    if res is None:
                        res = stage(i, off, nfr)
                    tok, got, want = res
                    self.t_io += time.perf_counter() - t
                    self.full.put((tok, got // frame_bytes, got))
                    if got < want:
                        break
            except BaseException as e:      # noqa: BLE001 - re-raised on the consumer's side
                self.err = e
            self.full.put(None)
        self.thr = threading.Thread(target=loop, name="crtfx-reader", daemon=True)
        if autostart:
            self.thr.start()

    def start(self):
        """autostart=False: the first read is issued here (the CLI times its pipeline from this point, with every staging slot already pinned)."""
        self.thr.start()

    def get(self):
        item = self.full.get()
        if self.err is not None:
            raise self.err
        return item

    def upload(self, tok, n: int, dst, stream):
        """Enqueue the host-to-device copy of the batch's first n frames into dst[:n] on `stream` (a torch stream)."""
        if isinstance(tok, _MapTok):
            self.rmap.copy(_HostDma.H2D, dst.data_ptr(), tok.off, n * self.frame_bytes, stream.cuda_stream)
        else:
            with self._torch.cuda.stream(stream):
                dst[:n].copy_(self._buf(tok)[:n], non_blocking=True)

    def release(self, tok):
        if isinstance(tok, _MapTok):
            if tok.nbytes:
                self.rmap.release(tok.off, tok.nbytes)
            self.free.put(tok.slot)
        else:
            self.free.put(tok)

    def close(self):
        self.free.put(None)
        self.thr.join(timeout=30)
        if self.rmap is not None:
            self.rmap.close()
        if self.mapped is not None:
            self.mapped.close()


class _Writer(_PinnedSlots):
    """A thread that finishes output batches behind the GPU.  `slot()` blocks until a destination is free and returns its token;
    `download(token, frames, src, stream)` enqueues the device-to-host copy; `put(token, frames, event, offset)` queues the batch for the
    thread, which waits for the event and
      staged   writes the pinned slot out (token = slot index; positional pwrite slices for a regular file, write() for a stream);
      mapped   (regular output file whose final size is known: `plan` = [(offset, bytes), ...]) has nothing left to write — the file was
               sized with ftruncate, mapped MAP_SHARED, and a helper thread registered each batch's windows with the HIP runtime ahead of
               the GPU, so the download DMA wrote the page cache itself; the thread only unregisters the windows.
    After the first write error nothing more is written: the remaining jobs are drained (their slots go back) and the first error is kept."""

    def __init__(self, fout, positional: bool, shape, frame_bytes: int, slots: int = 3, plan=None, io: str = "staged"):
        import os
        import queue
        import threading
        super().__init__(shape, slots)
        self.frame_bytes = frame_bytes
        self._os, self._closed = os, False
        try:
            self._fd = fout.fileno() if positional else None
        except (OSError, ValueError, AttributeError):
            self._fd = None
        self.free, self.work = queue.Queue(), queue.Queue()
        for i in range(slots):
            self.free.put(i)
        self.err, self.frames = None, 0
        self.t_wait = self.t_io = 0.0          # seconds this thread waited for downloads / spent writing
        self.rmap, self.ready, self.prep = None, None, None
        self.note = ""
        self.mapped_batches = 0
        self.t_prep = 0.0
        if positional and plan and io in ("mapped", "auto"):
            total = plan[-1][0] + plan[-1][1]
            try:
                os.ftruncate(fout.fileno(), total)
                self.rmap = _RegisteredMap(fout.fileno(), total, writable=True)
            except (OSError, ValueError, AttributeError) as e:
                self.rmap, self.note = None, f"output mapping refused ({e.__class__.__name__}): staged"
        if self.rmap is not None:
            self.ready = queue.Queue()
            self.tokens = threading.Semaphore(slots)      # batches registered ahead of / in flight on the GPU

            def prepare():
                for off, nbytes in plan:
                    self.tokens.acquire()
                    if self.stop_prep:
                        return
                    t = time.perf_counter()
                    ok = self.rmap.acquire(off, nbytes)
                    self.t_prep += time.perf_counter() - t
                    if not ok:
                        self.note = "hipHostRegister refused the output mapping: staged"
                        self.ready.put(None)           # from here on: pinned slots + pwrite into the (already sized) file
                        return
                    self.ready.put(_MapTok(off, nbytes, None))
                self.ready.put(None)
            self.stop_prep = False
            self.prep = threading.Thread(target=prepare, name="crtfx-out-prep", daemon=True)
            self.prep.start()
        else:
            for i in range(slots):
                self._buf(i)

        def loop():
            while True:
                job = self.work.get()
                if job is None:
                    return
                tok, n, ev, off = job
                try:
                    t = time.perf_counter()
                    ev.synchronize()
                    self.t_wait += time.perf_counter() - t
                    if isinstance(tok, _MapTok):
                        self.frames += n
                    elif self.err is None:          # after a write error: no further writes, the slots still go back
                        view = memoryview(self._buf(tok).numpy()).cast("B")[: n * frame_bytes]
                        t = time.perf_counter()
                        if positional:
                            _pwrite_full(fout.fileno(), view, off)
                        else:
                            fout.write(view)
                        self.t_io += time.perf_counter() - t
                        self.frames += n
                except BaseException as e:      # noqa: BLE001
                    if self.err is None:
                        self.err = e
                if isinstance(tok, _MapTok):
                    self.rmap.release(tok.off, tok.nbytes)
                    self.tokens.release()
                else:
                    self.free.put(tok)
        self.thr = threading.Thread(target=loop, name="crtfx-writer", daemon=True)
        self.thr.start()

    def slot(self):
        if self.err is not None:
            raise self.err
        if self.ready is not None:
            tok = self.ready.get()
            if tok is not None:
                self.mapped_batches += 1
                return tok
            self.ready = None                      # the plan is used up (a longer input than planned cannot happen) or registration failed
        return self.free.get()

    def download(self, tok, n: int, src, stream):
        """Enqueue the device-to-host copy of src[:n] into the batch's destination on `stream` (a torch stream)."""
        if isinstance(tok, _MapTok):
            self.rmap.copy(_HostDma.D2H, src.data_ptr(), tok.off, n * self.frame_bytes, stream.cuda_stream)
        else:
            with self._torch.cuda.stream(stream):
                self._buf(tok)[:n].copy_(src[:n], non_blocking=True)

    def put(self, tok, n: int, ev, off):
        self.work.put((tok, n, ev, off))

    def close(self):
        self.work.put(None)
        self.thr.join()
        if self.prep is not None:
            self.stop_prep = True
            for _ in range(len(self._bufs) + 1):
                self.tokens.release()
            self.prep.join(timeout=30)
        if self.rmap is not None:
            if self.mapped_batches and not self._closed:
                # the download DMA wrote MAP_SHARED pages of the output file directly: msync + fsync before the windows are unregistered and the
                # mapping goes, so that the frames' way to the disk does not hang on how the driver marked the pinned pages (INTEGRATION.md,
                # "--io mapped durability"); on tmpfs both calls return at once
                try:
                    self.rmap.map.flush()
                    if self._fd is not None:
                        self._os.fsync(self._fd)
                except (OSError, ValueError) as e:
                    if self.err is None:
                        self.err = e
            self.rmap.close()
        self._closed = True
        if self.err is not None:
            raise self.err
