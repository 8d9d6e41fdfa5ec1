"""Shared by test_ortho_overviews_host.py and ortho_overviews_gpu_child.py: the shapes, contents and band partitions of the
overview tests, and the rule of DESIGN.md §4.13 restated in numpy, level by level from the level before."""
import numpy as np

# (width, height): the expected (width, height) of the levels 1, 2, ...
SHAPES = {
    (1, 1): [],
    (2, 2): [],
    (2, 9): [],
    (3, 3): [(2, 2)],
    (64, 64): [(32, 32), (16, 16), (8, 8), (4, 4), (2, 2)],
    (65, 65): [(33, 33), (17, 17), (9, 9), (5, 5), (3, 3), (2, 2)],
    (130, 67): [(65, 34), (33, 17), (17, 9), (9, 5), (5, 3), (3, 2)],
    (129, 200): [(65, 100), (33, 50), (17, 25), (9, 13), (5, 7), (3, 4), (2, 2)],
    (1000, 5): [(500, 3), (250, 2)],
}
RGBA_CONTENTS = ["alpha_0", "alpha_255", "alpha_half", "one_valid", "alpha_mixed", "three_of_four_255"]
FLOAT_CONTENTS = ["nan_random", "nan_all", "nan_but_one", "large_halves"]
PARTITION_SHAPE = (129, 200)
PARTITIONS = {"one_feed": [200], "bands_64": [64, 64, 64, 8], "ragged": [1, 63, 70, 37, 29]}


def raster(content, width, height):
    """the level 0 of a content at a shape: (height, width, 4) uint8 or (height, width) float32"""
    rng = np.random.default_rng(sum(map(ord, content)) * 1000003 + width * 1009 + height)
    if content in RGBA_CONTENTS:
        r = rng.integers(0, 256, (height, width, 4), dtype=np.uint8)
        if content == "alpha_0":
            r[..., 3] = 0
        elif content == "alpha_255":
            r[..., 3] = 255
        elif content == "alpha_half":
            r[..., 3] = np.where(rng.random((height, width)) < 0.5, 255, 0)
        elif content == "one_valid":
            r[..., 3] = 0
            r[height // 2, width // 3, 3] = 255
        elif content == "alpha_mixed":
            r[..., 3] = rng.choice(np.array([0, 1, 128, 255], np.uint8), (height, width))
        elif content == "three_of_four_255":
            # colour 255 everywhere; in every 2 x 2 cell one pixel (a random one) has alpha 0, the others alpha 255
            r[..., :3] = 255
            r[..., 3] = 255
            off = rng.integers(0, 4, ((height + 1) // 2, (width + 1) // 2))
            yy, xx = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
            r[..., 3][(yy % 2) * 2 + xx % 2 == off[yy // 2, xx // 2]] = 0
        return r
    f = rng.normal(100.0, 30.0, (height, width)).astype(np.float32)
    if content == "nan_random":
        f[rng.random((height, width)) < 0.4] = np.nan
    elif content == "nan_all":
        f[:] = np.nan
    elif content == "nan_but_one":
        f[:] = np.nan
        f[height // 2, width // 2] = 3.25
        f[0, 0] = -7.5
    elif content == "large_halves":
        # 1e7 + {0, 0.5, 1, 1.5} rounded to float32 (whose spacing there is 1): a cell's sum of 2, 3 or 4 of them is exact
        # in double and not representable in float, so a float sum would round differently
        f = (1e7 + rng.choice(np.array([0, 0.5, 1, 1.5]), (height, width))).astype(np.float32)
        f = np.where(rng.random((height, width)) < 0.2, np.float32(np.nan), f).astype(np.float32)
    return f


def _cells(level):
    """the four cell planes (top-left, top-right, bottom-left, bottom-right) of a level padded to even sides, and whether
    each plane's pixel exists"""
    h, w = level.shape[:2]
    H, W = (h + 1) // 2, (w + 1) // 2
    pad = np.zeros((2 * H, 2 * W) + level.shape[2:], level.dtype)
    pad[:h, :w] = level
    exists = np.zeros((2 * H, 2 * W), bool)
    exists[:h, :w] = True
    planes = [pad[i::2, j::2] for i in (0, 1) for j in (0, 1)]
    return planes, [exists[i::2, j::2] for i in (0, 1) for j in (0, 1)]


def next_level(level):
    """one level from the one before by the rule, written independently of the library"""
    planes, exists = _cells(level)
    if level.dtype == np.uint8:
        m = sum(e.astype(np.int64) for e in exists)
        valid = [e & (p[..., 3] > 0) for p, e in zip(planes, exists)]
        n = sum(v.astype(np.int64) for v in valid)
        out = np.zeros(planes[0].shape, np.uint8)
        nn = np.maximum(n, 1)
        for c in range(3):
            s = sum(np.where(v, p[..., c].astype(np.int64), 0) for p, v in zip(planes, valid))
            out[..., c] = np.where(n > 0, (s + nn // 2) // nn, 0)
        a = sum(np.where(e, p[..., 3].astype(np.int64), 0) for p, e in zip(planes, exists))
        out[..., 3] = np.where(n > 0, (a + m // 2) // m, 0)
        return out
    valid = [e & ~np.isnan(p) for p, e in zip(planes, exists)]
    n = sum(v.astype(np.int64) for v in valid)
    s = np.zeros(planes[0].shape, np.float64)
    for p, v in zip(planes, valid):  # in the order top-left, top-right, bottom-left, bottom-right
        s = np.where(v, s + p.astype(np.float64), s)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = (s / n.astype(np.float64)).astype(np.float32)
    out[n == 0] = np.float32(np.nan)
    return out


def restated(level0):
    """[level 1, level 2, ...] of a raster by the numpy restatement: one level for every factor 2^k < min(width, height)"""
    h, w = level0.shape[:2]
    levels, cur, k = [], level0, 1
    while (1 << k) < min(w, h):
        cur = next_level(cur)
        levels.append(cur)
        k += 1
    return levels


def same(a, b):
    """equal as bits (float32: NaN payloads included), shapes included"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float32:
        return np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return np.array_equal(a, b)


def cases():
    """(name, content, width, height) of every shape x content"""
    return [(f"{c}_{w}x{h}", c, w, h) for (w, h) in SHAPES for c in RGBA_CONTENTS + FLOAT_CONTENTS]


def fed_in_bands(host, level0, rows_list, ctx=None, to_device=None):
    """the levels of level0 fed to a builder in bands of rows_list rows; complete_rows must be monotone and end whole"""
    h, w = level0.shape[:2]
    kind = host.OVERVIEW_RGBA8 if level0.dtype == np.uint8 else host.OVERVIEW_FLOAT32
    with host.OrthoOverviews(kind, w, h, ctx=ctx, on_device=to_device is not None) as b:
        row0, seen = 0, [0] * len(b.levels)
        for rows in rows_list:
            band = level0[row0:row0 + rows]
            b.feed(row0, to_device(band) if to_device is not None else band)
            row0 += rows
            now = [b.complete_rows(k + 1) for k in range(len(b.levels))]
            assert all(n >= s for n, s in zip(now, seen)), (now, seen)
            # a level's rows are complete as soon as the rows fed allow it
            have = row0
            for k, n in enumerate(now):
                prev_h = -(-h // (1 << k))
                have = -(-prev_h // 2) if have == prev_h else have // 2
                assert n == have, (k + 1, n, have)
            seen = now
        levels = b.finish()
        assert [b.complete_rows(k + 1) for k in range(len(levels))] == [int(l.shape[0]) for l in levels]
        return [l if isinstance(l, np.ndarray) else l.cpu().numpy() for l in levels]
