"""Images, shapes and an independent numpy restatement of the load stage's thumbnail (csrc/thumbnail.hpp) for
test_thumbnail_host.py and the GPU scenarios of thumbnails_gpu_child.py.  The restatement shares only host.lab_convert (the
project's one colour definition) with the code under test: its tables, its float32 sums tap by tap in table order and its
integer cells are written here."""
import math

import numpy as np

from opencalibration_amd import host

# name -> (width, height, batch); "general": pixel counts that are no (50 n)^2, "integer": those that are
SHAPES = {
    "general_1400x1050_batch3": (1400, 1050, 3),   # 24.2 taps per axis; the batch catches per-image offsets
    "general_odd_1013x757": (1013, 757, 1),        # rows of 3039 bytes: no multiple of 4, 17.5 taps
    "general_small_173x131": (173, 131, 1),        # 3 taps, cells that straddle
    "general_4000x3000": (4000, 3000, 1),          # 69.3 taps: the only shape whose staging window is a whole 12 Mpx row
    "integer_180x125": (180, 125, 1),              # n = 3, 42 x 60, a partial bottom row of cells
    "integer_250x90": (250, 90, 1),                # n = 3, 30 x 83, an unused source column
    "integer_320x125": (320, 125, 1),              # n = 4
    "integer_100x100": (100, 100, 1),              # n = 2
}
CPU_SHAPES = [k for k in SHAPES if k != "general_4000x3000"]


def images(name):
    """The seeded batch of a shape, (batch, h, w, 3) uint8: image i is kind i mod 3 of a smooth gradient, a gradient plus
    noise, and uniformly random colours (a table gather's worst case)."""
    w, h, batch = SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    out = np.zeros((batch, h, w, 3), np.uint8)
    x, y = np.arange(w, dtype=np.float32)[None, :, None] / w, np.arange(h, dtype=np.float32)[:, None, None] / h
    for i in range(batch):
        kind = i % 3 if batch > 1 else {"general_odd_1013x757": 1, "general_4000x3000": 1}.get(name, 2)
        if kind == 2:
            out[i] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            continue
        a = rng.uniform(20, 235, (3, 3)).astype(np.float32)
        g = a[None, None, :, 0] + (a[:, 1] - a[:, 0]) * x + (a[:, 2] - a[:, 0]) * y  # (h, w, 3)
        if kind == 1:
            g = g + rng.integers(0, 41, g.shape, dtype=np.uint8).astype(np.float32) - 20
        out[i] = np.clip(np.rint(g), 0, 255).astype(np.uint8)
    return out


def size_restated(width, height):
    """(rows, cols, 1 / scale): cv::resize's dsize = saturate_cast<int>(ssize * scale), ties to even"""
    scale = 50.0 / math.sqrt(float(width * height))
    return int(np.rint(height * scale)), int(np.rint(width * scale)), 1.0 / scale


def area_table_restated(ssize, dsize, scale):
    """computeResizeAreaTab: per destination the source indices and float32 weights, in table order"""
    taps = []
    for d in range(dsize):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, ssize - f1)
        s1, s2 = math.ceil(f1), min(math.floor(f2), ssize - 1)
        s1 = min(s1, s2)
        t = []
        if s1 - f1 > 1e-3:
            t.append((s1 - 1, np.float32((s1 - f1) / cell)))
        t += [(s, np.float32(1.0 / cell)) for s in range(s1, s2)]
        if f2 - s2 > 1e-3:
            t.append((s2, np.float32(min(min(f2 - s2, 1.0), cell) / cell)))
        taps.append(t)
    return taps


def _padded(taps):
    most = max(len(t) for t in taps)
    idx = np.zeros((len(taps), most), np.int64)
    wgt = np.zeros((len(taps), most), np.float32)  # a padding tap adds +0.0f * S[0]: the sum is unchanged
    for d, t in enumerate(taps):
        for k, (s, a) in enumerate(t):
            idx[d, k], wgt[d, k] = s, a
    return idx, wgt


def resize_general_restated(lab, rows, cols, inv_scale):
    h, w, _ = lab.shape
    xi, xa = _padded(area_table_restated(w, cols, inv_scale))
    yi, ya = _padded(area_table_restated(h, rows, inv_scale))
    S = lab.astype(np.float32)
    buf = np.zeros((h, cols, 3), np.float32)
    for k in range(xi.shape[1]):
        buf = buf + S[:, xi[:, k], :] * xa[None, :, k, None]
    out = np.zeros((rows, cols, 3), np.float32)
    for k in range(yi.shape[1]):
        out = out + buf[yi[:, k]] * ya[:, k, None, None]
    assert buf.dtype == np.float32 and out.dtype == np.float32
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def resize_integer_restated(lab, rows, cols, n):
    """ResizeAreaFast: complete cells scale their integer sum by the float 1 / (n n), partial ones divide by their count"""
    h, w, _ = lab.shape
    out = np.zeros((rows, cols, 3), np.uint8)
    inv = np.float32(1.0) / np.float32(n * n)
    for dy in range(rows):
        for dx in range(cols):
            cell = lab[dy * n:min(dy * n + n, h), dx * n:min(dx * n + n, w)].astype(np.int64)
            total, count = cell.sum((0, 1)), cell.shape[0] * cell.shape[1]
            v = total.astype(np.float32) * inv if count == n * n else total.astype(np.float32) / np.float32(count)
            out[dy, dx] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return out


def lab_of(bgr):
    """host.lab_convert of an (h, w, 3) image, each distinct colour converted once"""
    flat = bgr.reshape(-1, 3)
    codes = flat[:, 0].astype(np.uint32) | flat[:, 1].astype(np.uint32) << 8 | flat[:, 2].astype(np.uint32) << 16
    uniq, inverse = np.unique(codes, return_inverse=True)
    u = np.stack([uniq & 255, uniq >> 8 & 255, uniq >> 16 & 255], -1).astype(np.uint8)
    return host.lab_convert(u, "bgr2lab8")[inverse].reshape(bgr.shape)


def thumbnail_restated(bgr):
    """(rows, cols, 3) R G B of one (h, w, 3) BGR image"""
    h, w, _ = bgr.shape
    rows, cols, inv_scale = size_restated(w, h)
    n = int(np.rint(inv_scale))
    lab = lab_of(bgr)
    if abs(inv_scale - n) < np.finfo(np.float64).eps:
        small = resize_integer_restated(lab, rows, cols, n)
    else:
        small = resize_general_restated(lab, rows, cols, inv_scale)
    return host.lab_convert(small.reshape(-1, 3), "lab82bgr").reshape(rows, cols, 3)[..., ::-1]


_cpu = {}


def cpu_route(name):
    """host.image_thumbnails of a shape's batch on the CPU route: computed once, shared, left unchanged"""
    if name not in _cpu:
        _cpu[name] = host.image_thumbnails(images(name))
        _cpu[name].setflags(write=False)
    return _cpu[name]
