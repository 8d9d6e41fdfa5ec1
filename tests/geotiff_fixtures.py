"""The rasters and crafted payloads of the GeoTIFF tests (test_geotiff_host.py, geotiff_gpu_child.py): computed once, shared,
left unchanged."""
import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PAYLOAD, SEGMENT, ROW = 1 << 20, 16384, 2048
GEO = dict(min_x=431000.5, max_y=5411000.25, gsd=0.05, epsg=32632)


def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def ramp(h, w):
    x = np.arange(w, dtype=np.uint32)[None, :] + 3 * np.arange(h, dtype=np.uint32)[:, None]
    return np.stack([x & 255, (x >> 1) & 255, (x >> 2) & 255, np.full_like(x, 255)], -1).astype(np.uint8)


@functools.lru_cache(None)
def rgba(name):
    """width x height: one 1 x 1, 512 x 512, 513 x 511, 1100 x 700 (six tiles) and the photograph tiled to 600 x 600"""
    rng = np.random.default_rng(7)
    if name == "one_pixel":
        return _ro(np.array([[[9, 8, 7, 255]]], np.uint8))
    if name == "zeros":
        return _ro(np.zeros((700, 1100, 4), np.uint8))
    if name == "constant":
        return _ro(np.full((512, 512, 4), 77, np.uint8))
    if name == "ramp":
        return _ro(ramp(511, 513))
    if name == "half_zero":  # the right part zero: tile column 1 partly, tile column 2 wholly
        r = ramp(700, 1100)
        r[:, 600:] = 0
        return _ro(r)
    if name == "noise":
        return _ro(rng.integers(0, 256, (512, 512, 4), dtype=np.uint8))
    if name == "photo":
        from PIL import Image

        ph = np.asarray(Image.open(os.path.join(HERE, "golden", "jpeg_decode", "sample_test2.jpg")).convert("RGBA"))
        return _ro(np.tile(ph, (-(-600 // ph.shape[0]), -(-600 // ph.shape[1]), 1))[:600, :600])
    raise KeyError(name)


RGBA = ("one_pixel", "zeros", "constant", "ramp", "half_zero", "noise", "photo")
COMPRESSIBLE = ("zeros", "constant", "ramp", "half_zero", "photo")


@functools.lru_cache(None)
def dsm():
    """1100 x 700 float32: a smooth surface, NaN regions, tile (0, 2) all NaN, a -0.0, and a strip whose bit patterns wrap in
    the difference"""
    y, x = np.mgrid[0:700, 0:1100].astype(np.float32)
    d = (100 + 0.01 * x + 0.02 * y + np.sin(x / 37) * np.cos(y / 23)).astype(np.float32)
    d[40:90, 100:400] = np.nan
    d[:512, 1024:] = np.nan
    d[600, 5] = -0.0
    d[650, 0:64] = np.array([1, 0xFF7FFFFF] * 32, np.uint32).view(np.float32)
    return _ro(d)


def quiet(n, at=0):
    """n bytes of 64 values that match neither 4 nor 2 048 bytes back: nothing but literals"""
    p = np.arange(at, at + n, dtype=np.int64)
    return (((p >> 2) * 7 + (p & 3) * 3 + (p >> 11) * 5) & 63).astype(np.uint8)


@functools.lru_cache(None)
def crafted():
    """(names, (n, 1 MiB) payloads): the predicted bytes themselves, for deflate_tiles"""
    rng = np.random.default_rng(11)
    out = {}
    # the first segment: 17 values in Fibonacci proportion, 4 180 bytes, shuffled; zeros behind
    fib = [1, 1]
    while len(fib) < 17:
        fib.append(fib[-1] + fib[-2])
    assert sum(fib) == 4180
    p = np.zeros(PAYLOAD, np.uint8)
    p[:4180] = rng.permutation(np.repeat(np.arange(1, 18, dtype=np.uint8), fib))
    p[SEGMENT:] = quiet(PAYLOAD - SEGMENT, SEGMENT)
    out["fibonacci"] = p
    # a segment with a single distinct byte among quiet ones
    p = quiet(PAYLOAD)
    p[3 * SEGMENT:4 * SEGMENT] = 7
    out["single_byte_segment"] = p
    # a run of equal bytes across a segment's end: the match stops at the end, the next block starts with its own
    p = quiet(PAYLOAD)
    p[5 * SEGMENT - 300:5 * SEGMENT + 300] = 9
    out["match_across_segments"] = p
    # this payload's last row is the next one's first row: distance 2 048 in a tile's first row would reach into it
    p = quiet(PAYLOAD)
    out["before_first_row"] = p
    q = quiet(PAYLOAD, 12345 * 4)
    q[:ROW] = p[-ROW:]
    q[ROW:2 * ROW] = q[:ROW]  # and the second row repeats the first: here distance 2 048 is right
    out["first_row"] = q
    names = tuple(out)
    return names, _ro(np.stack([out[k] for k in names]))
