"""Shared by test_jpeg_host.py, test_gpu_jpeg.py, jpeg_gpu_child.py and scripts/make_jpeg_golden.py: the shapes, the seeded
contents and the golden cases of the JPEG texture tests.  Nothing here goes through the library."""
import os

import numpy as np

# (height, width): one pixel; one block; one MCU; an MCU with a dummy block to the right / below; sizes around the 8- and
# 16-pixel grids, among them the ones whose last chroma row repeats (8 x 8, 8 x 16, 24 x 40); a few MCUs in both directions
SHAPES = [(1, 1), (2, 2), (8, 8), (16, 16), (8, 16), (16, 8), (7, 25), (25, 7), (9, 17), (17, 9), (15, 15), (24, 40), (40, 24),
          (31, 33), (33, 47), (48, 64), (64, 80)]
CONTENTS = ["noise", "ramp", "flat", "checker"]
QUALITIES = [1, 10, 50, 75, 90, 95, 100]
QUALITY_SHAPES = [(1, 1), (8, 24), (17, 33), (32, 48)]
# Flat 255 at 16 x 16: the six blocks' DC differences and EOBs by hand; every further MCU adds a2 8a 28 00 (32 bits)
FLAT_SCAN_16 = bytes.fromhex("fdfca28a2803")
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_texture")
# (content, height, width, quality, seed) of the committed files
GOLDEN = [("noise", 33, 47, 95, 5), ("flat", 16, 16, 95, 0), ("flat", 48, 64, 95, 0), ("ramp", 8, 8, 95, 0), ("ramp", 8, 16, 95, 0),
          ("ramp", 24, 40, 95, 0), ("ramp", 7, 25, 95, 0), ("noise", 1, 1, 95, 1), ("checker", 32, 48, 50, 0), ("noise", 17, 33, 1, 2),
          ("noise", 17, 33, 100, 2), ("ramp", 31, 33, 75, 0)]


def noise(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)


def ramp(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(5 * x + 3 * y) % 256, (2 * x + 7 * y) % 256, (x + y) % 256], -1).astype(np.uint8)


def flat(h, w):
    return np.full((h, w, 3), 255, np.uint8)


def checker(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.repeat(np.where((x + y) % 2 == 0, 100, 156)[..., None], 3, -1).astype(np.uint8)


def content(kind, h, w, seed=0):
    """the (h, w, 3) uint8 raster of a content"""
    return {"noise": lambda: noise(h, w, seed), "ramp": lambda: ramp(h, w), "flat": lambda: flat(h, w),
            "checker": lambda: checker(h, w)}[kind]()


def rgba_of(rgb, alpha_seed=7):
    """the raster with an alpha channel of noise behind it: the encoder must not read it"""
    a = np.random.default_rng(alpha_seed).integers(0, 256, rgb.shape[:2] + (1,)).astype(np.uint8)
    return np.ascontiguousarray(np.concatenate([rgb, a], -1))


def golden_name(case):
    kind, h, w, q, seed = case
    return f"{kind}_{h}x{w}_q{q}_s{seed}.jpg"


def golden_bytes(case):
    with open(os.path.join(GOLDEN_DIR, golden_name(case)), "rb") as f:
        return f.read()


def scan_of(jpeg):
    """the entropy-coded data of a baseline file written by these encoders: behind the SOS header, ahead of EOI"""
    at = jpeg.index(b"\xff\xda\x00\x0c")
    assert jpeg.endswith(b"\xff\xd9")
    return jpeg[at + 14:-2]


def zrl_symbols(jpeg):
    """the number of ZRL symbols of the file: decodes the scan's symbols with the file's own Huffman tables"""
    tables, at = {}, 2
    while jpeg[at:at + 2] != b"\xff\xda":
        marker, length = jpeg[at + 1], int.from_bytes(jpeg[at + 2:at + 4], "big")
        if marker == 0xC4:
            cls, bits, vals = jpeg[at + 4], jpeg[at + 5:at + 21], jpeg[at + 21:at + 2 + length]
            codes, code, k = {}, 0, 0
            for ln in range(1, 17):
                for _ in range(bits[ln - 1]):
                    codes[(ln, code)] = vals[k]
                    code, k = code + 1, k + 1
                code <<= 1
            tables[cls] = codes
        if marker == 0xC0:
            h, w = int.from_bytes(jpeg[at + 5:at + 7], "big"), int.from_bytes(jpeg[at + 7:at + 9], "big")
        at += 2 + length
    data = scan_of(jpeg).replace(b"\xff\x00", b"\xff")
    bits = "".join(f"{b:08b}" for b in data)
    pos, zrl = 0, 0

    def symbol(table):
        nonlocal pos
        code, ln = 0, 0
        while True:
            code, ln, pos = code << 1 | int(bits[pos]), ln + 1, pos + 1
            if (ln, code) in table:
                return table[(ln, code)]

    for _ in range(-(-h // 16) * -(-w // 16)):
        for b in range(6):
            c = 0 if b < 4 else 1
            category = symbol(tables[c])  # (symbol moves pos: read it before adding to it)
            pos += category
            k = 1
            while k < 64:
                s = symbol(tables[0x10 | c])
                if s == 0:
                    break
                zrl += s == 0xF0
                k += (s >> 4) + 1
                pos += s & 15
    return zrl
