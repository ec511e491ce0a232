"""The picture on the CPU: the numpy restatement (tests/render_ref.py) against
the float64 check (tests/render_checks.py) on every case the GPU tests use,
the colour map at its corners, wrong rules that the check has to catch, and the
PNG writer against a decoder written here."""
import struct
import zlib

import numpy as np
import pytest

from cfd2_amd import image
from tests import render_cases as RC
from tests import render_checks as K
from tests import render_ref as R

F = np.float32


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_restatement_passes_f64_check(name):
    mesh, W, H, box, full, owner = RC.case(name)
    vx, vy, off, idx = RC.polygons_of(RC.CASES[name][0])
    r = K.assert_owner_map(vx, vy, off, idx, full, owner, cap=1.0 if name in RC.UNCAPPED else 0.05)  # no violation
    print(name, "cells", len(off) - 1, "covered", int((owner != R.NONE).sum()), "of", W * H, "undecided share", r["share"],
          "eps", r["eps"])
    if name == "outside":
        assert not (owner != R.NONE).any()
    if name == "obstacle":  # the hole of the obstacle is background, the channel around it is not
        cy, cx = H // 2, int(1.0 / 3.0 * W)
        assert owner[cy, cx] == R.NONE and owner[2, cx] != R.NONE
    if name == "big":  # many cells per pixel: each pixel's owner is one of ~8 candidates
        assert len(off) - 1 >= 65536


def test_every_pixel_inside_the_channel_is_owned():
    vx, vy, off, idx = RC.polygons_of("rect")
    owner = R.owner_map(vx, vy, off, idx, R.View(40, 20, (0.1, 0.1, 0.9, 0.4)))
    assert (owner != R.NONE).all()
    full = R.owner_map(vx, vy, off, idx, R.View(64, 32, R.bounds(vx, vy, idx)))
    assert (full != R.NONE).all()  # the closed tests leave no crack between the cells


def test_colour_map():
    c = R.colour(np.array([0.0, 0.25, 0.5, 1.0, -3.0, 7.0, np.nan], F), 0.0, 1.0)
    assert c.tolist() == [[0, 0, 255, 255], [0, 128, 128, 255], [0, 255, 0, 255], [255, 0, 0, 255],
                          [0, 0, 255, 255], [255, 0, 0, 255], [0, 0, 0, 255]]
    # a degenerate range: safe = 1, so val - lo is the normalised value
    d = R.colour(np.array([2.0, 2.5, 3.0], F), 2.0, 2.0)
    assert d.tolist() == [[0, 0, 255, 255], [0, 255, 0, 255], [255, 0, 0, 255]]
    # every byte is (uint8)(c * 255 + 0.5) of the f32 channel
    t = np.linspace(0, 1, 1001).astype(F)
    g = R.colour(t, 0.0, 1.0)
    low = t < F(0.5)
    s = np.where(low, t * F(2), (t - F(0.5)) * F(2)).astype(F)
    assert np.array_equal(g[low, 1], (s[low] * F(255) + F(0.5)).astype(np.uint8))
    assert np.array_equal(g[~low, 0], (s[~low] * F(255) + F(0.5)).astype(np.uint8))


def test_auto_range_and_keys():
    v = np.array([0.5, -0.0, 0.0, np.nan, -2.0, np.inf], F)
    lo, hi = R.auto_range(v)
    assert lo == F(-2.0) and hi == F(np.inf)
    lo, hi = R.auto_range(np.array([0.0, -0.0], F))
    assert np.signbit(lo) and not np.signbit(hi)  # the keys order -0 below +0
    assert R.auto_range(np.array([np.nan, np.nan], F)) == (F(0), F(1))
    k = R.value_key(v[~np.isnan(v)])
    assert np.array_equal(R.key_value(k).view(np.uint32), v[~np.isnan(v)].view(np.uint32))


def test_shade_background_and_nan():
    owner = np.array([[0, R.NONE], [1, 2]], np.uint32)
    img, (lo, hi) = R.render(owner, np.array([1.0, np.nan, 3.0], F))
    assert (lo, hi) == (F(1), F(3))
    assert img.tolist() == [[[0, 0, 255, 255], [0, 0, 0, 0]], [[0, 0, 0, 255], [255, 0, 0, 255]]]


# ---- wrong rules: the check has to catch them --------------------------------
def _square(x0, y0, s):
    return [(x0, y0), (x0 + s, y0), (x0 + s, y0 + s), (x0, y0 + s)]


def _poly_arrays(polys):
    vx = np.array([p[0] for poly in polys for p in poly], np.float64)
    vy = np.array([p[1] for poly in polys for p in poly], np.float64)
    off = np.cumsum([0] + [len(p) for p in polys])
    return vx, vy, off, np.arange(off[-1])


def test_smallest_index_rule_is_caught():
    # cell 1 lies over the upper right quarter of cell 0: the largest index owns the overlap
    vx, vy, off, idx = _poly_arrays([_square(0.0, 0.0, 1.0), _square(0.5, 0.5, 0.5)])
    box = (0.0, 0.0, 1.0, 1.0)
    good = R.owner_map(vx, vy, off, idx, R.View(16, 16, box))
    assert (good[:8, 8:] == 1).all() and (good[8:, :] == 0).all()
    K.assert_owner_map(vx, vy, off, idx, box, good)
    bad = R.owner_map(vx, vy, off, idx, R.View(16, 16, box), rule="smallest")
    r = K.check_owner_map(vx, vy, off, idx, box, bad)
    assert r["bad_higher"] == 64 and r["bad_owner"] == 0


def test_open_test_is_caught():
    # an 8 x 8 image of the unit square: the centres with i + j = 7 lie exactly on the fan's diagonal
    vx, vy, off, idx = _poly_arrays([_square(0.0, 0.0, 1.0)])
    box = (0.0, 0.0, 1.0, 1.0)
    good = R.owner_map(vx, vy, off, idx, R.View(8, 8, box))
    assert (good == 0).all()
    K.assert_owner_map(vx, vy, off, idx, box, good)
    bad = R.owner_map(vx, vy, off, idx, R.View(8, 8, box), closed=False)
    assert (bad == R.NONE).sum() == 8  # the crack along the diagonal
    r = K.check_owner_map(vx, vy, off, idx, box, bad)
    assert r["bad_background"] == 8


def test_wrong_owner_and_shifted_map_are_caught():
    mesh, W, H, box, full, owner = RC.case("obstacle")
    vx, vy, off, idx = RC.polygons_of("obstacle")
    shifted = np.roll(owner, 3, axis=1)
    r = K.check_owner_map(vx, vy, off, idx, full, shifted)
    assert r["bad_owner"] > 0
    painted = np.array(owner)
    painted[painted == R.NONE] = 0  # the hole painted with cell 0
    assert K.check_owner_map(vx, vy, off, idx, full, painted)["bad_owner"] > 0


def test_degenerate_polygons_own_nothing():
    # a two-vertex "cell", a zero-area triangle and a clockwise square (both windings are drawn)
    polys = [[(0.1, 0.1), (0.9, 0.9)], [(0.0, 0.0), (0.5, 0.5), (1.0, 1.0)], _square(0.0, 0.0, 1.0)[::-1]]
    vx, vy, off, idx = _poly_arrays(polys)
    owner = R.owner_map(vx, vy, off, idx, R.View(8, 8, (0.0, 0.0, 1.0, 1.0)))
    assert (owner == 2).all()


# ---- the PNG writer -----------------------------------------------------------
def _png_decode(data):
    """a minimal decoder: chunks with their CRCs, zlib, the five scanline filters (8-bit RGBA)"""
    assert data[:8] == image.PNG_SIGNATURE
    pos, chunks = 8, []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(kind + body) & 0xFFFFFFFF
        chunks.append((kind, body))
        pos += 12 + n
    assert [k for k, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, ctype, comp, filt, lace) == (8, 6, 0, 0, 0)
    raw = zlib.decompress(b"".join(b for k, b in chunks if k == b"IDAT"))
    stride, bpp = 4 * w, 4
    assert len(raw) == h * (stride + 1)
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.int64)
    for j in range(h):
        ft, line = raw[j * (stride + 1)], np.frombuffer(raw, np.uint8, stride, j * (stride + 1) + 1).astype(np.int64)
        cur = np.zeros(stride, np.int64)
        for k in range(stride):
            a = cur[k - bpp] if k >= bpp else 0
            b, c = prev[k], (prev[k - bpp] if k >= bpp else 0)
            if ft == 0:
                pred = 0
            elif ft == 1:
                pred = a
            elif ft == 2:
                pred = b
            elif ft == 3:
                pred = (a + b) // 2
            else:
                pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            cur[k] = (line[k] + pred) & 255
        out[j], prev = cur, cur
    return out.reshape(h, w, 4)


def test_write_png_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (13, 31, 4), dtype=np.uint8)
    img[0, 0] = (0, 0, 0, 0)
    path = tmp_path / "frame.png"
    image.write_png(path, img)
    assert np.array_equal(_png_decode(path.read_bytes()), img)
    one = np.array([[[1, 2, 3, 255]]], np.uint8)
    assert np.array_equal(_png_decode(image.png_bytes(one)), one)
    with pytest.raises(ValueError):
        image.write_png(path, img[:, :, :3])
    with pytest.raises(ValueError):
        image.write_png(path, img.astype(np.float32))


def test_write_ppm(tmp_path):
    img = np.array([[[255, 0, 0, 255], [9, 9, 9, 0]], [[0, 255, 0, 255], [0, 0, 255, 255]]], np.uint8)
    path = tmp_path / "frame.ppm"
    image.write_ppm(path, img)
    data = path.read_bytes()
    assert data.startswith(b"P6\n2 2\n255\n")
    assert data[len(b"P6\n2 2\n255\n"):] == bytes([255, 0, 0, 255, 255, 255, 0, 255, 0, 0, 0, 255])
