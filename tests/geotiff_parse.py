"""A small TIFF reader for the GeoTIFF tests: header, IFD chain, tags and tile arrays of little-endian classic and BigTIFF files,
and the tiles of a level inflated with zlib and un-predicted.  It knows only what host.GeoTiffWriter writes."""
import struct
import zlib

import numpy as np

TILE, PAYLOAD, MAX_STREAM = 512, 1 << 20, 1048667
TYPES = {1: "B", 2: "c", 3: "H", 4: "I", 12: "d", 16: "Q"}


def parse(data):
    """[{tag: tuple of values (bytes for ASCII)}, ...] per IFD, and whether the file is BigTIFF"""
    data = bytes(data)
    assert data[:2] == b"II"
    magic = struct.unpack_from("<H", data, 2)[0]
    big = magic == 43
    assert magic in (42, 43)
    if big:
        assert struct.unpack_from("<HH", data, 4) == (8, 0)
        at = struct.unpack_from("<Q", data, 8)[0]
    else:
        at = struct.unpack_from("<I", data, 4)[0]
    ifds = []
    while at:
        assert at % 2 == 0 and at < len(data)
        n = struct.unpack_from("<Q" if big else "<H", data, at)[0]
        at += 8 if big else 2
        tags, last = {}, 0
        for _ in range(n):
            tag, typ = struct.unpack_from("<HH", data, at)
            count = struct.unpack_from("<Q" if big else "<I", data, at + 4)[0]
            field = at + (12 if big else 8)
            size = struct.calcsize("<" + TYPES[typ]) * count
            if size > (8 if big else 4):
                field = struct.unpack_from("<Q" if big else "<I", data, field)[0]
                assert field % 2 == 0
            values = struct.unpack_from(f"<{count}{TYPES[typ]}", data, field)
            tags[tag] = b"".join(values) if typ == 2 else values
            assert tag > last, "tags ascend"
            last = tag
            at += 20 if big else 12
        at = struct.unpack_from("<Q" if big else "<I", data, at)[0]
        ifds.append(tags)
    return ifds, big


def tiles(data, ifd):
    """[(offset, count, stream or None)] of an IFD's tiles in order"""
    return [(o, c, bytes(data[o:o + c]) if c else None) for o, c in zip(ifd[324], ifd[325])]


def unpredict(payload, is_float):
    """a tile's (512, 512) uint32 pixels from its predicted 1 MiB"""
    if is_float:
        return np.cumsum(np.frombuffer(payload, "<u4").reshape(TILE, TILE), axis=1, dtype=np.uint32)
    b = np.cumsum(np.frombuffer(payload, np.uint8).reshape(TILE, TILE, 4), axis=1, dtype=np.uint8)
    return np.ascontiguousarray(b).view("<u4").reshape(TILE, TILE)


def predict(tile_u32, is_float):
    """the predicted 1 MiB (uint8) of a (512, 512) uint32 tile"""
    if is_float:
        p = tile_u32.copy()
        p[:, 1:] = tile_u32[:, 1:] - tile_u32[:, :-1]
        return p.view(np.uint8).reshape(-1)
    b = np.ascontiguousarray(tile_u32).view(np.uint8).reshape(TILE, TILE, 4)
    p = b.copy()
    p[:, 1:] = b[:, 1:] - b[:, :-1]
    return p.reshape(-1)


def as_u32(raster):
    """(h, w) uint32 view of an RGBA8 or float32 raster"""
    raster = np.ascontiguousarray(raster)
    return raster.view("<u4").reshape(raster.shape[0], raster.shape[1])


def padded_tiles(raster):
    """the raster's tiles, zero-padded to 512 x 512, as (ty, tx, (512, 512) uint32) in file order"""
    px = as_u32(raster)
    h, w = px.shape
    th, tw = -(-h // TILE), -(-w // TILE)
    pad = np.zeros((th * TILE, tw * TILE), np.uint32)
    pad[:h, :w] = px
    return [(ty, tx, pad[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE]) for ty in range(th) for tx in range(tw)]


def check_level(data, ifd, raster, sparse_zero_ok=False):
    """Every tile of the IFD inflates (zlib) to 1 MiB that un-predicts to the raster's zero-padded pixels, no stream exceeds
    the stored form; returns the list of (ty, tx) of the tiles with offset 0 and count 0"""
    is_float = raster.dtype == np.float32
    want = padded_tiles(raster)
    got = tiles(data, ifd)
    assert len(got) == len(want), (len(got), len(want))
    assert ifd[256] == (raster.shape[1],) and ifd[257] == (raster.shape[0],)
    missing = []
    for (ty, tx, px), (o, c, stream) in zip(want, got):
        if c == 0:
            assert o == 0 and sparse_zero_ok and not px.any(), (ty, tx)
            missing.append((ty, tx))
            continue
        assert o % 2 == 0 and 0 < c <= MAX_STREAM, (ty, tx, o, c)
        payload = zlib.decompress(stream)
        assert len(payload) == PAYLOAD
        assert np.array_equal(unpredict(payload, is_float), px), (ty, tx)
    return missing
