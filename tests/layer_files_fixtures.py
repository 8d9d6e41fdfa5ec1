"""Rasters and an independent reader for the layers and cameras GeoTIFFs (the reference's
createMultiBandGeoTIFF, src/ortho/ortho.cpp:969-1008).  A raster pair is layer-major as ortho_layers leaves it: bgra
(L, h, w, 4) uint8 and camera_id (L, h, w) uint64.  The reader here knows nothing of the library: the IFD by geotiff_parse,
zlib.decompress on every tile, the predictor undone with numpy's cumsum at the stride of the sample count, the samples
de-interleaved.  Everything is computed once and handed out read-only."""
import io
import zlib

import numpy as np

import geotiff_parse as P

TILE = 512
SIZES = [(1, 1), (511, 3), (512, 512), (513, 513), (1030, 520)]  # width x height
LAYERS = [1, 2]
CONTENTS = ["zero", "noise", "layered"]
STEPS = [None, 1, 7, 511]  # fed whole, row by row, in bands of 7 and of 511 rows
# four node ids: two with a non-zero high word, one of them with a zero low word; 0 stands outside the valid region
IDS = np.array([0x0000000100000000, 0x9E3779B97F4A7C15, 0x00000000DEADBEEF, 0x000000000000002A], np.uint64)
GEO = dict(min_x=-12.5, max_y=40.25, gsd=0.05, epsg=32632)
LAYERS8, CAMERAS32 = 2, 3  # host.GEOTIFF_LAYERS8, host.GEOTIFF_CAMERAS32: the numbers are part of the C interface

_rasters = {}


def rasters(content, w, h, L):
    """(bgra (L, h, w, 4) uint8, camera_id (L, h, w) uint64), read-only"""
    key = (content, w, h, L)
    if key not in _rasters:
        rng = np.random.default_rng(1000 * w + 10 * h + L)
        if content == "zero":
            bgra, ids = np.zeros((L, h, w, 4), np.uint8), np.zeros((L, h, w), np.uint64)
        elif content == "noise":
            bgra = rng.integers(0, 256, (L, h, w, 4), dtype=np.uint8)
            ids = rng.integers(0, 1 << 63, (L, h, w), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (L, h, w), dtype=np.uint64)
        else:
            y, x = np.mgrid[0:h, 0:w].astype(np.float64)
            bgra, ids = np.zeros((L, h, w, 4), np.uint8), np.zeros((L, h, w), np.uint64)
            for l in range(L):
                cx, cy = w * (0.45 + 0.1 * l), h * (0.5 - 0.07 * l)
                dx, dy = (x - cx) / max(0.48 * w, 1.0), (y - cy) / max(0.46 * h, 1.0)
                ang = np.arctan2(dy, dx)
                ragged = 1.0 + 0.12 * np.sin(7 * ang + l) + 0.03 * rng.random((h, w))  # a ragged edge, another per layer
                valid = dx * dx + dy * dy < ragged
                colour = np.stack([96 + 80 * np.sin(x / 97.0 + l), 128 + 100 * np.cos(y / 131.0), 60 + 0.1 * (x + y) % 190,
                                   np.full((h, w), 255.0)], -1)
                bgra[l][valid] = colour[valid].astype(np.uint8)
                which = ((2 * x // max(w, 1)).astype(int) + 2 * (2 * y // max(h, 1)).astype(int) + l) % 4
                ids[l][valid] = IDS[which][valid]
        bgra.setflags(write=False), ids.setflags(write=False)
        _rasters[key] = (bgra, ids)
    return _rasters[key]


def pixel_bytes(kind, L):
    return (4 if kind == LAYERS8 else 8) * L


def stored_bytes(n):
    return 2 + n + 5 * -(-n // 65535) + 4


def interleaved(kind, raster):
    """the file's view of a layer-major raster: (h, w, samples) uint8 (B G R A per layer) or uint32 (low, high per layer)"""
    if kind == LAYERS8:
        L, h, w, _ = raster.shape
        return np.ascontiguousarray(raster.transpose(1, 2, 0, 3)).reshape(h, w, 4 * L)
    L, h, w = raster.shape
    words = np.ascontiguousarray(raster.astype("<u8")).view("<u4").reshape(L, h, w, 2)
    return np.ascontiguousarray(words.transpose(1, 2, 0, 3)).reshape(h, w, 2 * L)


def layer_major(kind, samples, L):
    """the inverse of interleaved"""
    h, w, _ = samples.shape
    if kind == LAYERS8:
        return np.ascontiguousarray(samples.reshape(h, w, L, 4).transpose(2, 0, 1, 3))
    words = np.ascontiguousarray(samples.reshape(h, w, L, 2).transpose(2, 0, 1, 3))
    return words.view("<u8").reshape(L, h, w).astype(np.uint64)


def padded_tiles(kind, raster):
    """[(ty, tx, (512, 512, samples) tile, zero-padded)] in file order"""
    s = interleaved(kind, raster)
    h, w, n = s.shape
    th, tw = -(-h // TILE), -(-w // TILE)
    pad = np.zeros((th * TILE, tw * TILE, n), s.dtype)
    pad[:h, :w] = s
    return [(ty, tx, pad[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE]) for ty in range(th) for tx in range(tw)]


def predict(tile):
    """numpy's horizontal differencing of a (512, 512, samples) tile: its payload bytes"""
    p = tile.copy()
    p[:, 1:] = tile[:, 1:] - tile[:, :-1]  # wraps in the samples' own width
    return p.tobytes()


def unpredict(payload, kind, L):
    n = (4 if kind == LAYERS8 else 2) * L
    dt = np.uint8 if kind == LAYERS8 else np.dtype("<u4")
    return np.cumsum(np.frombuffer(payload, dt).reshape(TILE, TILE, n), axis=1, dtype=dt)


def decode(data, kind, L):
    """(the layer-major raster of a file, [(ty, tx)] of the tiles left out, [stream sizes of the tiles written], the IFD)"""
    ifds, _ = P.parse(data)
    assert len(ifds) == 1, "no overview levels"
    t = ifds[0]
    w, h = t[256][0], t[257][0]
    n = (4 if kind == LAYERS8 else 2) * L
    assert t[277] == (n,) and t[322] == (TILE,) and t[323] == (TILE,)
    th, tw = -(-h // TILE), -(-w // TILE)
    assert len(t[324]) == len(t[325]) == th * tw
    full = np.zeros((th * TILE, tw * TILE, n), np.uint8 if kind == LAYERS8 else np.dtype("<u4"))
    missing, sizes = [], []
    for k, (o, c) in enumerate(zip(t[324], t[325])):
        ty, tx = divmod(k, tw)
        if c == 0:
            assert o == 0
            missing.append((ty, tx))
            continue
        assert o % 2 == 0 and c <= stored_bytes(TILE * TILE * pixel_bytes(kind, L)), (ty, tx, o, c)
        payload = zlib.decompress(bytes(data[o:o + c]))
        assert len(payload) == TILE * TILE * pixel_bytes(kind, L)
        full[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE] = unpredict(payload, kind, L)
        sizes.append(c)
    return layer_major(kind, np.ascontiguousarray(full[:h, :w]), L), missing, sizes, t


def written(host, kind, raster, step=None, ctx=None, on_device=False, **kw):
    """the file of a layer-major raster (numpy, or a CUDA tensor with on_device) fed in bands of `step` rows (None: whole)"""
    L, h, w = (int(v) for v in raster.shape[:3])
    f = io.BytesIO()
    with host.GeoTiffWriter(f, kind, w, h, num_layers=L, ctx=ctx, on_device=on_device, **kw) as wr:
        for r in range(0, h, step or h):
            band = raster[:, r:r + (step or h)]
            wr.feed(r, band.contiguous() if on_device else band)
        wr.finish()
    return f.getvalue()


def build_file(kind, raster, levels=(1, 6, 9, 0), sparse=True, geo=None, big=False):
    """A layers or cameras file by numpy's predictor and zlib.compress, nothing of the library: tile k at level
    levels[k % len] - level 0 is zlib's stored form - and, with sparse, the all-zero tiles at offset 0 / count 0"""
    import struct

    out = bytearray(b"II+\0\x08\0\0\0" + bytes(8) if big else b"II*\0" + bytes(4))
    inline, fmt_off = (8, "<Q") if big else (4, "<I")

    def put(data):
        if len(out) & 1:
            out.append(0)
        at = len(out)
        out.extend(data)
        return at

    L, h, w = raster.shape[:3]
    n = (4 if kind == LAYERS8 else 2) * L
    offs, cnts = [], []
    for k, (_, _, t) in enumerate(padded_tiles(kind, raster)):
        if sparse and not t.any():
            offs.append(0), cnts.append(0)
            continue
        z = zlib.compress(predict(t), levels[k % len(levels)])
        offs.append(put(z)), cnts.append(len(z))
    S, L4, D, L8 = 3, 4, 12, 16
    tags = {256: (L4, [w]), 257: (L4, [h]), 258: (S, [8 if kind == LAYERS8 else 32] * n), 259: (S, [8]), 262: (S, [1]), 277: (S, [n]),
            284: (S, [1]), 317: (S, [2]), 322: (S, [TILE]), 323: (S, [TILE]), 324: (L8 if big else L4, offs), 325: (L4, cnts),
            338: (S, [0] * (n - 1)), 339: (S, [1] * n)}
    if geo is not None:
        tags[33550] = (D, [geo["gsd"], geo["gsd"], 0.0])
        tags[33922] = (D, [0.0, 0.0, 0.0, geo["min_x"], geo["max_y"], 0.0])
        tags[34735] = (S, [1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, int(geo["epsg"])])
    dtypes = {S: "<u2", L4: "<u4", D: "<f8", L8: "<u8"}
    entries = []
    for tag in sorted(tags):
        typ, values = tags[tag]
        data = np.asarray(values).astype(dtypes[typ]).tobytes()
        field = data.ljust(inline, b"\0") if len(data) <= inline else struct.pack(fmt_off, put(data))
        entries.append(struct.pack("<HH", tag, typ) + struct.pack(fmt_off, len(values)) + field)
    at = put(struct.pack("<Q" if big else "<H", len(entries)) + b"".join(entries) + bytes(inline))
    out[8 if big else 4:(8 if big else 4) + inline] = struct.pack(fmt_off, at)
    return bytes(out)
