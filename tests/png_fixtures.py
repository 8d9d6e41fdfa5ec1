"""The images of the PNG tests (test_png_host.py, png_gpu_child.py): computed once, shared, left unchanged; and the PNG
chunk helpers the tests read and rewrite files with."""
import functools
import struct
import zlib

import numpy as np

import geotiff_fixtures as G

SEGMENT = 16384


def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def ramp(h, w, c):
    x = np.arange(w, dtype=np.uint32)[None, :] * 2 + 3 * np.arange(h, dtype=np.uint32)[:, None]
    planes = [x & 255, (x >> 1) & 255, (x >> 2) & 255, np.full_like(x, 255)]
    return np.stack(planes[:c], -1).astype(np.uint8) if c > 1 else (x & 255).astype(np.uint8)


def noisy(a, seed):
    rng = np.random.default_rng(seed)
    return (a.astype(np.int32) + rng.integers(0, 5, a.shape)).astype(np.uint8)  # amplitude 4


@functools.lru_cache(None)
def image(name):
    rng = np.random.default_rng(23)
    if name == "one_gray":
        return _ro(np.array([[200]], np.uint8))
    if name == "one_rgb":
        return _ro(np.array([[[1, 2, 3]]], np.uint8))
    if name == "one_rgba":
        return _ro(np.array([[[9, 8, 7, 255]]], np.uint8))
    if name == "thumb_ramp":  # thumbnail size: 58 x 43, stride 175
        return _ro(ramp(43, 58, 3))
    if name == "thumb_noisy":
        return _ro(noisy(ramp(43, 58, 3), 1))
    if name == "five_by_three":
        return _ro(rng.integers(0, 256, (3, 5, 3), dtype=np.uint8))
    if name == "gray_127x128":  # F = 16 384: exactly one segment
        return _ro(noisy(ramp(128, 127, 1), 2))
    if name == "gray_16384x1":  # F = 16 385: a second segment of one byte
        return _ro(noisy(ramp(1, 16384, 1), 3))
    if name == "gray_32767x2":  # stride 32 768: the up candidate at its limit
        a = noisy(ramp(2, 32767, 1), 4)
        a[1, 1000:9000] = a[0, 1000:9000]  # after filtering the rows differ; runs of equal filtered bytes above each other follow
        a[:, 20000:24000] = 17
        return _ro(a)
    if name == "gray_32768x2":  # no up candidate
        a = noisy(ramp(2, 32768, 1), 4)
        a[:, 20000:24000] = 17
        return _ro(a)
    if name == "gray_noise_300":  # stored: two stored blocks
        return _ro(rng.integers(0, 256, (300, 300), dtype=np.uint8))
    if name == "rgba_ramp":
        return _ro(ramp(768, 1024, 4))
    if name == "rgba_noisy":
        return _ro(noisy(ramp(768, 1024, 4), 5))
    if name == "rgba_photo":
        ph = np.asarray(G.rgba("photo"))
        return _ro(np.tile(ph, (2, 2, 1))[:768, :1024])
    if name == "constant_rows":  # a run crosses a segment's end: rows of one value each, 40 rows of 1 001 bytes
        return _ro(np.repeat((np.arange(40, dtype=np.uint8) * 37)[:, None], 1000, 1))
    if name in NARROW:  # strides of 2, 3, 6 and 10 bytes: every alignment of the byte above, columns that repeat down the image
        w, h, c = NARROW[name]
        a = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        a[h // 3:] = a[h // 3]  # equal rows: Up gives zeros, None gives matches a stride back
        a[::7] = rng.integers(0, 256, (len(range(0, h, 7)), w, c), dtype=np.uint8)
        return _ro(a[..., 0] if c == 1 else a)
    raise KeyError(name)


NARROW = dict(gray_1x700=(1, 700, 1), gray_2x500=(2, 500, 1), gray_5x400=(5, 400, 1), rgb_3x300=(3, 300, 3))
SMALL = tuple(NARROW) + ("one_gray", "one_rgb", "one_rgba", "thumb_ramp", "thumb_noisy", "five_by_three", "gray_127x128", "gray_16384x1",
         "gray_32767x2", "gray_32768x2", "gray_noise_300", "constant_rows")
LARGE = ("rgba_ramp", "rgba_noisy", "rgba_photo")
ALL = SMALL + LARGE
COMPRESSIBLE_LARGE = ("gray_32767x2", "gray_32768x2") + LARGE  # every compressible fixture with F >= 65 536: the size bound applies


def swapped(a):
    """what a file written with bgr=True holds"""
    if a.ndim == 3 and a.shape[2] >= 3:
        return a[..., [2, 1, 0] + list(range(3, a.shape[2]))]
    return a


def payload_bytes(a):
    h = a.shape[0]
    return h * (1 + a[0].size)


def stored_bytes(F):
    return 2 + F + 5 * -(-F // 65535) + 4


def thumb_batch(n):
    """n copies of the noisy thumbnail with a per-copy offset added"""
    base = image("thumb_noisy").astype(np.int32)
    return [(base + 3 * k).astype(np.uint8) for k in range(n)]


# ---- chunks ----------------------------------------------------------------------------------------------------------------
SIGNATURE = b"\x89PNG\r\n\x1a\n"


def chunks(data):
    """[(type, body, crc, offset of the chunk)] of a PNG file"""
    assert data[:8] == SIGNATURE
    out, at = [], 8
    while at < len(data):
        n, = struct.unpack(">I", data[at:at + 4])
        out.append((data[at + 4:at + 8], data[at + 8:at + 8 + n], struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0], at))
        at += 12 + n
    assert at == len(data)
    return out


def chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def rebuilt(parts):
    return SIGNATURE + b"".join(chunk(k, b) for k, b in parts)


def ihdr(w, h, depth, colour, interlace=0):
    return struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, interlace)


def idat_of(data):
    return b"".join(b for k, b, _, _ in chunks(data) if k == b"IDAT")
