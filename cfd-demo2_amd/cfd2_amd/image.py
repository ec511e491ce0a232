"""Keeping a frame of ``GpuSolver.render`` without any imaging package: PNG and
PPM writers over ``zlib`` and ``struct`` of the standard library.
"""
from __future__ import annotations

import struct
import zlib

import numpy as np

PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _rgba(rgba) -> np.ndarray:
    a = np.ascontiguousarray(rgba)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 4 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("expected an (H, W, 4) uint8 RGBA image")
    return a


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def png_bytes(rgba, level: int = 6) -> bytes:
    """The image as an 8-bit RGBA PNG (colour type 6, no interlace), every
    scanline with filter type 0 (None): the pixel bytes are stored as they are."""
    a = _rgba(rgba)
    h, w = a.shape[:2]
    rows = np.empty((h, 1 + 4 * w), dtype=np.uint8)
    rows[:, 0] = 0
    rows[:, 1:] = a.reshape(h, 4 * w)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)
    return (PNG_SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) +
            _chunk(b"IEND", b""))


def write_png(path, rgba, level: int = 6) -> None:
    """Write ``rgba`` ((H, W, 4) uint8, row 0 the top) to ``path`` as a PNG."""
    data = png_bytes(rgba, level)
    with open(path, "wb") as fh:
        fh.write(data)


def write_ppm(path, rgba, background=(255, 255, 255)) -> None:
    """Write ``rgba`` to ``path`` as a binary PPM (P6).  PPM has no alpha:
    pixels with alpha 0 (off the mesh) take ``background``."""
    a = _rgba(rgba)
    h, w = a.shape[:2]
    rgb = a[:, :, :3].copy()
    rgb[a[:, :, 3] == 0] = np.asarray(background, dtype=np.uint8)
    with open(path, "wb") as fh:
        fh.write(b"P6\n%d %d\n255\n" % (w, h))
        fh.write(rgb.tobytes())
