"""`Cube` — a 3D colour LUT as a `.cube` file holds it (the format of Resolve, ffmpeg's `lut3d=`, OpenColorIO's bakes), and its quantised
table as the 3D LUT stage takes it (include/crtfx_lut3d.h, pythoncrt_amd/lut3d.py).

    cube = Cube.load("pq2020_to_709.cube")       # or Cube(size, values[N, N, N, 3]) / Cube.identity(33)
    table = cube.quantise()                      # uint16 [N, N, N, 3], quarter codes 0..1020: rint_to_even(1020 * clip(v, 0, 1))

The reader takes `TITLE`, `#` comments and blank lines, `LUT_3D_SIZE N` (2..65), optional `DOMAIN_MIN 0 0 0` / `DOMAIN_MAX 1 1 1`, then
N^3 rows of three floats, red fastest.  It refuses, with a ValueError that names the line: `LUT_1D_SIZE`, any other domain, N outside
2..65, a wrong number of rows, a non-finite value, an unknown keyword.  Entries and results of the stage are quarter codes, so a cube's
precision here is 10 bits."""
from __future__ import annotations

import numpy as np

QMAX, MIN_N, MAX_N = 1020, 2, 65


class Cube:
    """`values` is float64 [N, N, N, 3] indexed [b][g][r][c]: red fastest, as the rows of the file run."""

    def __init__(self, size: int, values, title: str = ""):
        if isinstance(size, bool) or int(size) != size or not MIN_N <= int(size) <= MAX_N:
            raise ValueError(f"a cube's size must be an integer in {MIN_N}..{MAX_N}, got {size!r}")
        self.size = int(size)
        v = np.asarray(values, dtype=np.float64)
        if v.size != self.size ** 3 * 3:
            raise ValueError(f"a cube of size {self.size} holds {self.size ** 3} rows of three values, got {v.size} values")
        if not np.isfinite(v).all():
            raise ValueError("a cube's values must be finite")
        self.values = np.ascontiguousarray(v.reshape(self.size, self.size, self.size, 3))
        self.title = str(title)

    @classmethod
    def identity(cls, size: int) -> "Cube":
        """The cube that maps every colour to itself: entry [b][g][r] = (r, g, b) / (N - 1)."""
        if isinstance(size, bool) or int(size) != size or not MIN_N <= int(size) <= MAX_N:
            raise ValueError(f"a cube's size must be an integer in {MIN_N}..{MAX_N}, got {size!r}")
        n = int(size)
        b, g, r = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
        return cls(n, np.stack([r, g, b], axis=-1) / float(n - 1), title="identity")

    @classmethod
    def load(cls, path) -> "Cube":
        """Read a `.cube` file.  ValueError names the file and the line; OSError is the file system's."""
        with open(path, "r", encoding="utf-8", errors="replace") as f:
            return cls.parse(f, name=str(path))

    @classmethod
    def parse(cls, lines, name: str = "<cube>") -> "Cube":
        """`lines`: an iterable of text lines (an open file, text.splitlines())."""
        size, title, rows, first_row, no = None, "", [], 0, 0

        def bad(no, why):
            return ValueError(f"{name}, line {no}: {why}")
        for no, raw in enumerate(lines, 1):
            line = raw.strip()
            if not line or line.startswith("#"):
                continue
            word = line.split()[0]
            try:
                float(word)                                     # "nan" and "inf" are numbers: a row, refused as one
                keyword = False
            except ValueError:
                keyword = word[0].isalpha() or word[0] == "_"
            if keyword:
                rest = line[len(word):].strip()
                if rows:
                    raise bad(no, f"keyword {word} behind the table's first row (line {first_row})")
                if word == "TITLE":
                    title = rest.strip('"')
                elif word == "LUT_3D_SIZE":
                    if size is not None:
                        raise bad(no, "a second LUT_3D_SIZE")
                    try:
                        size = int(rest)
                    except ValueError:
                        raise bad(no, f"LUT_3D_SIZE {rest!r} is not an integer") from None
                    if not MIN_N <= size <= MAX_N:
                        raise bad(no, f"LUT_3D_SIZE {size} outside {MIN_N}..{MAX_N}")
                elif word == "LUT_1D_SIZE":
                    raise bad(no, "LUT_1D_SIZE: a 1D LUT; only 3D cubes (LUT_3D_SIZE) are applied")
                elif word in ("DOMAIN_MIN", "DOMAIN_MAX"):
                    want = 0.0 if word == "DOMAIN_MIN" else 1.0
                    try:
                        got = [float(t) for t in rest.split()]
                    except ValueError:
                        got = []
                    if len(got) != 3 or any(g != want for g in got):
                        raise bad(no, f"{word} {rest}: only the domain 0 0 0 .. 1 1 1 is taken")
                else:
                    raise bad(no, f"unknown keyword {word}")
                continue
            if size is None:
                raise bad(no, "a table row in front of LUT_3D_SIZE")
            parts = line.split()
            try:
                vals = [float(t) for t in parts]
            except ValueError:
                raise bad(no, f"{line!r} is not a row of three numbers") from None
            if len(vals) != 3:
                raise bad(no, f"a row holds three values, got {len(vals)}")
            if not all(np.isfinite(vals)):
                raise bad(no, f"a non-finite value in {line!r}")
            if len(rows) == size ** 3:
                raise bad(no, f"more than the {size ** 3} rows of LUT_3D_SIZE {size}")
            if not rows:
                first_row = no
            rows.append(vals)
        if size is None:
            raise ValueError(f"{name}: no LUT_3D_SIZE line")
        if len(rows) != size ** 3:
            raise ValueError(f"{name}, line {no}: the file ends after {len(rows)} of the {size ** 3} rows of LUT_3D_SIZE {size}")
        return cls(size, np.array(rows, dtype=np.float64), title=title)

    def quantise(self) -> np.ndarray:
        """uint16 [N, N, N, 3]: rint_to_even(1020 * min(max(v, 0), 1)) in float64 — the table crtfx_lut3d_create takes."""
        return np.rint(1020.0 * np.minimum(np.maximum(self.values, 0.0), 1.0)).astype(np.uint16)


def as_cube(cube, name: str = "cube") -> Cube:
    """A `Cube` from what a keyword was given: a Cube, or a path.  ValueError: unreadable or malformed."""
    if isinstance(cube, Cube):
        return cube
    import os
    if not isinstance(cube, (str, os.PathLike)):
        raise ValueError(f"{name} must be a path to a .cube file or a Cube, got {cube!r}")
    try:
        return Cube.load(cube)
    except OSError as e:
        raise ValueError(f"{name}={str(cube)!r}: cannot read the cube ({e})") from None
