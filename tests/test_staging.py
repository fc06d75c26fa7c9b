"""pythoncrt_amd.staging — the host I/O staging behind the CLI: positional and mapped file I/O, pipe sizing, registered file mappings.
No GPU."""
import os

import numpy as np

from pythoncrt_amd import staging


def test_positional_file_io_helpers(tmp_path, monkeypatch):
    """staging._pread_full / _pwrite_full: sliced, threaded positional I/O equals one plain read / write — offsets, a short file, sizes that
    are not a multiple of the slice."""
    import numpy as np
    monkeypatch.setattr(staging, "_IO_SLICE", 1000)                      # many slices on a small file
    data = np.random.default_rng(5).integers(0, 256, 12345, dtype=np.uint8).tobytes()
    src = tmp_path / "src.bin"
    src.write_bytes(data)
    fd = os.open(src, os.O_RDONLY)
    try:
        buf = bytearray(5000)
        assert staging._pread_full(fd, memoryview(buf), 2345) == 5000 and bytes(buf) == data[2345:7345]
        buf = bytearray(4000)                                        # runs past the end of the file: the contiguous prefix only
        got = staging._pread_full(fd, memoryview(buf), 10000)
        assert got == 2345 and bytes(buf[:got]) == data[10000:]
        buf = bytearray(300)                                         # a single slice
        assert staging._pread_full(fd, memoryview(buf), 0) == 300 and bytes(buf) == data[:300]
    finally:
        os.close(fd)
    dst = tmp_path / "dst.bin"
    fd = os.open(dst, os.O_WRONLY | os.O_CREAT)
    try:
        staging._pwrite_full(fd, memoryview(data)[:7000], 0)
        staging._pwrite_full(fd, memoryview(data)[7000:], 7000)
        staging._pwrite_full(fd, memoryview(b""), 0)
    finally:
        os.close(fd)
    assert dst.read_bytes() == data
    with open(src, "rb") as f:
        assert staging._seekable(f)
    r, w = os.pipe()
    try:
        with os.fdopen(r, "rb") as pr:
            assert not staging._seekable(pr)
    finally:
        os.close(w)


def test_mapped_input_reads_like_the_file(tmp_path):
    """staging._MappedInput — the regular-file input path (mmap + memcpy on the I/O threads instead of read(2)): whole batches, the short
    last batch, offsets past the end, slices larger and smaller than the I/O slice, an empty file."""
    import os
    data = np.random.default_rng(0).integers(0, 256, 40_000_003, dtype=np.uint8)
    path = tmp_path / "in.rgb"
    path.write_bytes(data.tobytes())
    fd = os.open(path, os.O_RDONLY)
    m = staging._MappedInput(fd)
    dst = np.empty(33_000_000, dtype=np.uint8)           # > 16 MiB: split over the pool
    assert m.read_into(dst, 0) == dst.size and np.array_equal(dst, data[:dst.size])
    assert m.read_into(dst, 33_000_000) == 7_000_003 and np.array_equal(dst[:7_000_003], data[33_000_000:])
    assert m.read_into(dst, data.size) == 0 and m.read_into(dst, data.size + 5) == 0
    small = np.empty(1000, dtype=np.uint8)
    assert m.read_into(small, 12345) == 1000 and np.array_equal(small, data[12345:13345])
    m.close()
    os.close(fd)
    empty = tmp_path / "empty.rgb"
    empty.write_bytes(b"")
    fd = os.open(empty, os.O_RDONLY)
    m = staging._MappedInput(fd)
    assert m.map is None and m.read_into(small, 0) == 0
    m.close()
    os.close(fd)


def test_cli_pipes_get_the_large_buffer():
    """staging._grow_pipe: F_SETPIPE_SZ on both ends of a pipe (1 MiB, or the most the kernel grants); 0 for a regular file."""
    from pythoncrt_amd import staging
    r, wfd = os.pipe()
    try:
        with os.fdopen(r, "rb", buffering=0) as fr, os.fdopen(wfd, "wb", buffering=0) as fw:
            got = staging._grow_pipe(fw)
            assert got >= 65536 and staging._grow_pipe(fr) == got          # one buffer, seen from both ends
        with open(__file__, "rb") as f:
            assert staging._grow_pipe(f) == 0
    finally:
        pass


def test_registered_map_windows(tmp_path, monkeypatch):
    """staging._RegisteredMap (the --io mapped path) without a GPU: hipHostRegister / Unregister / MemcpyAsync replaced by recorders.  Windows sit on a
    fixed grid, a window two batches share is registered once and unregistered when the second one lets go, a refused registration leaves nothing
    registered for that call, and a copy is issued window by window (the runtime rejects one that runs across two registrations)."""
    calls = []
    refuse = set()

    class FakeDma:
        H2D, D2H = 1, 2

        @staticmethod
        def register(ptr, n):
            if ptr in refuse:
                return False
            calls.append(("reg", ptr, n))
            return True

        @staticmethod
        def unregister(ptr):
            calls.append(("unreg", ptr))

        @staticmethod
        def copy(dst, src, n, kind, stream):
            calls.append(("copy", dst, src, n, kind))
    monkeypatch.setattr(staging, "_HostDma", FakeDma)
    monkeypatch.setattr(staging._RegisteredMap, "WIN", 64 * 1024)
    win = 64 * 1024
    size = 5 * win + 1234
    path = tmp_path / "f.bin"
    path.write_bytes(os.urandom(size))
    fd = os.open(path, os.O_RDONLY)
    try:
        m = staging._RegisteredMap(fd, size, writable=False)
        base = m.base
        # batch A: bytes [10 000, 150 000) = windows 0, 1, 2
        assert m.acquire(10_000, 140_000)
        assert [c for c in calls if c[0] == "reg"] == [("reg", base, win), ("reg", base + win, win), ("reg", base + 2 * win, win)]
        # batch B: [150 000, 300 000) = windows 2, 3, 4: window 2 is shared and not registered again
        calls.clear()
        assert m.acquire(150_000, 150_000)
        assert [c[1] for c in calls if c[0] == "reg"] == [base + 3 * win, base + 4 * win]
        # the copy of batch B runs window by window, contiguous on both sides
        calls.clear()
        m.copy(FakeDma.H2D, 1 << 40, 150_000, 150_000, 0)
        cp = [c for c in calls if c[0] == "copy"]
        assert [c[3] for c in cp] == [3 * win - 150_000, win, 300_000 - 4 * win] and sum(c[3] for c in cp) == 150_000
        assert cp[0][1] == 1 << 40 and cp[0][2] == base + 150_000 and cp[1][1] == (1 << 40) + cp[0][3] and cp[1][2] == base + 3 * win
        calls.clear()
        m.copy(FakeDma.D2H, 1 << 40, 10_000, 100, 0)                      # device -> file: destination is the mapping
        assert calls == [("copy", base + 10_000, 1 << 40, 100, FakeDma.D2H)]
        # releasing A frees windows 0 and 1; window 2 stays for B
        calls.clear()
        m.release(10_000, 140_000)
        assert calls == [("unreg", base), ("unreg", base + win)]
        calls.clear()
        m.release(150_000, 150_000)
        assert calls == [("unreg", base + 2 * win), ("unreg", base + 3 * win), ("unreg", base + 4 * win)] and m.ref == {}
        # the last window is clipped to the mapping's page-rounded length
        calls.clear()
        assert m.acquire(5 * win + 10, 1000)
        assert calls == [("reg", base + 5 * win, m.maplen - 5 * win)] and m.maplen % 4096 == 0 and m.maplen >= size
        m.release(5 * win + 10, 1000)
        # a refused window: what this call had registered is rolled back, what another batch holds stays
        assert m.acquire(0, 10)
        calls.clear()
        refuse.add(base + 2 * win)
        assert not m.acquire(10, 2 * win + 10)                             # windows 0 (held), 1 (new), 2 (refused)
        assert calls == [("reg", base + win, win), ("unreg", base + win)] and m.ref == {0: 1}
        m.close()
        assert ("unreg", base) in calls and m.ref == {}
    finally:
        os.close(fd)
