"""What the GeoTIFF reading tests share (test_geotiff_read_host.py, geotiff_read_gpu_child.py): a small TIFF builder, an LSB
bit writer for hand-assembled deflate blocks, and the stream zoo.  Nothing binary is committed: everything is generated from
seeds, computed once, shared and left unchanged.  zlib is the reference for every stream: what it gives is what an accepted
stream must give, and what it refuses must be refused."""
import functools
import struct
import zlib

import numpy as np

RING, CHUNK = 65536, 16384        # the device route's LDS window and flush chunk (csrc/geotiff_read.hip)
SIZES = (0, 1, 255, 1024, 65535, 65536, 65537, 1 << 20)


# ---- payloads and zlib's streams ---------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def payload(kind, n):
    rng = np.random.default_rng(1000 + n % 9973)
    if kind == "zeros":
        return bytes(n)
    if kind == "noise":
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == "ramp":
        return ((np.arange(n) // 7 + rng.integers(0, 3, n)) & 255).astype(np.uint8).tobytes()
    if kind == "text":
        period = bytes((37 * i + i // 5) % 96 + 32 for i in range(300))
        return (period * (n // 300 + 1))[:n]
    raise KeyError(kind)


KINDS = ("zeros", "noise", "ramp", "text")


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, flush=None):
    """zlib's stream of data; flush: a flush mode applied in the middle, which leaves an empty stored block there"""
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    if flush is None:
        return c.compress(data) + c.flush()
    half = len(data) // 2
    return c.compress(data[:half]) + c.flush(flush) + c.compress(data[half:]) + c.flush()


VARIANTS = (("level0", dict(level=0)), ("level1", dict(level=1)), ("level6", dict(level=6)), ("level9", dict(level=9)),
            ("fixed", dict(strategy=zlib.Z_FIXED)), ("huffman_only", dict(strategy=zlib.Z_HUFFMAN_ONLY)), ("rle", dict(strategy=zlib.Z_RLE)),
            ("wbits9", dict(wbits=9)), ("wbits15", dict(wbits=15)), ("sync_flush", dict(flush=zlib.Z_SYNC_FLUSH)),
            ("full_flush", dict(flush=zlib.Z_FULL_FLUSH)))


# ---- hand-assembled blocks -----------------------------------------------------------------------------------------------------
class Bits:
    """bits LSB first; Huffman codes go in most significant bit first, as RFC 1951 3.1.1 packs them"""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, k):
        self.acc |= (v & ((1 << k) - 1)) << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, k):
        self.put(int(format(c, f"0{k}b")[::-1], 2) if k else 0, k)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def raw(self, data):
        self.align()
        self.out += data

    def bytes(self):
        self.align()
        return bytes(self.out)


LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


def fixed_lit(b, s):
    if s < 144:
        b.code(0x30 + s, 8)
    elif s < 256:
        b.code(0x190 + s - 144, 9)
    elif s < 280:
        b.code(s - 256, 7)
    else:
        b.code(0xC0 + s - 280, 8)


def length_symbol(n):
    k = max(i for i in range(29) if LEN_BASE[i] <= n and (i < 28 or n == 258))
    return 257 + k, LEN_EXTRA[k], n - LEN_BASE[k]


def distance_symbol(d):
    k = max(i for i in range(30) if DIST_BASE[i] <= d)
    return k, DIST_EXTRA[k], d - DIST_BASE[k]


def fixed_block(b, tokens, final=True):
    """tokens: an int (a literal), (length, distance), or ("sym", s) / ("dsym", length, s) for symbols as they stand"""
    b.put(1 if final else 0, 1)
    b.put(1, 2)
    for t in tokens:
        if isinstance(t, int):
            fixed_lit(b, t)
        elif t[0] == "sym":
            fixed_lit(b, t[1])
        else:
            n, d = (t[1], None) if t[0] == "dsym" else t
            s, eb, ev = length_symbol(n)
            fixed_lit(b, s)
            b.put(ev, eb)
            if d is None:
                b.code(t[2], 5)
            else:
                ds, eb, ev = distance_symbol(d)
                b.code(ds, 5)
                b.put(ev, eb)
    fixed_lit(b, 256)


def stored_block(b, data, final=False, nlen=None):
    b.put(1 if final else 0, 1)
    b.put(0, 2)
    b.align()
    b.put(len(data), 16)
    b.put((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
    b.raw(data)


def stored_run(b, data):
    """data in stored blocks, none of them final"""
    for at in range(0, len(data), 65535):
        stored_block(b, data[at:at + 65535])


def canonical(lens):
    """{symbol: (code, length)} of {symbol: length}"""
    code, out = 0, {}
    for n in range(1, 16):
        for s in sorted(k for k, v in lens.items() if v == n):
            out[s] = (code, n)
            code += 1
        code <<= 1
    return out


CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
CL_PLAIN = {s: 4 for s in range(16)}                                   # the lengths 0 .. 15 as they stand: a complete code
CL_WITH_16 = {**{s: 4 for s in range(15)}, 15: 5, 16: 5}               # and the repeat


def dynamic_block(b, lit_lens, dist_lens, tokens, final=True, hlit=None, hdist=None, cl_lens=CL_PLAIN, sequence=None, eob=True):
    """A dynamic block from {symbol: length} of both codes; sequence: the code-length symbols as they go out - ints, or
    (16, extra) and the like - instead of one plain length per code"""
    hlit = max(257, max(lit_lens) + 1) if hlit is None else hlit
    hdist = max(1, max(dist_lens, default=0) + 1) if hdist is None else hdist
    b.put(1 if final else 0, 1)
    b.put(2, 2)
    b.put(hlit - 257, 5)
    b.put(hdist - 1, 5)
    b.put(19 - 4, 4)
    for s in CL_ORDER:
        b.put(cl_lens.get(s, 0), 3)
    cl = canonical(cl_lens)
    if sequence is None:
        sequence = [lit_lens.get(s, 0) for s in range(hlit)] + [dist_lens.get(s, 0) for s in range(hdist)]
    for t in sequence:
        s, extra = (t, None) if isinstance(t, int) else t
        b.code(*cl[s])
        if extra is not None:
            b.put(extra, {16: 2, 17: 3, 18: 7}[s])
    lit, dist = canonical(lit_lens), canonical(dist_lens)
    for t in tokens:
        if isinstance(t, int):
            b.code(*lit[t])
        else:
            s, eb, ev = length_symbol(t[0])
            b.code(*lit[s])
            b.put(ev, eb)
            ds, eb, ev = distance_symbol(t[1])
            b.code(*dist[ds])
            b.put(ev, eb)
    if eob:
        b.code(*lit[256])


def zlib_wrap(b, data, header=b"\x78\x9c", adler=None, tail=b""):
    """the zlib stream around the deflate bits of b, which inflate to data"""
    return header + b.bytes() + struct.pack(">I", zlib.adler32(data) if adler is None else adler) + tail


def inflate_by_zlib(z):
    """(bytes, True) if zlib takes the whole of z as one stream, else (None, False)"""
    d = zlib.decompressobj()
    try:
        out = d.decompress(z)
    except zlib.error:
        return None, False
    return (out, True) if d.eof and not d.unused_data else (None, False)


def _pattern(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@functools.lru_cache(None)
def hand_cases():
    """{name: (stream, payload)}: what zlib 1.2.11's deflate never writes - it stays below distance 32 507 - and the corners
    of the device route's ring.  Every one is checked against zlib's inflate where it is made."""
    out = {}

    def far(prefix_len, name):
        p = _pattern(prefix_len, prefix_len)
        b = Bits()
        stored_run(b, p)
        fixed_block(b, [(258, 32768), 65, (100, 32768)])
        data = bytearray(p)
        for n, d in ((258, 32768), (0, 0), (100, 32768)):
            if n == 0:
                data.append(65)
            for _ in range(n):
                data.append(data[-d])
        out[name] = (zlib_wrap(b, bytes(data)), bytes(data))

    far(32768, "distance_32768")
    far(RING - 100, "distance_32768_target_crosses_the_wrap")
    far(RING + 32768 - 100, "distance_32768_source_crosses_the_wrap")
    far(3 * RING - 7, "distance_32768_third_lap")
    b = Bits()
    fixed_block(b, [66] + [(258, 1)] * 300)
    out["dist_1_len_258"] = (zlib_wrap(b, b"B" * (1 + 258 * 300)), b"B" * (1 + 258 * 300))
    b = Bits()
    fixed_block(b, [97, 98, (3, 2), (258, 5), (258, 3), (257, 7)])
    data = bytearray(b"ab")
    for n, d in ((3, 2), (258, 5), (258, 3), (257, 7)):
        for _ in range(n):
            data.append(data[-d])
    out["len_3_dist_2"] = (zlib_wrap(b, bytes(data)), bytes(data))
    # HDIST = 1 and a distance code of length zero: a block of literals alone; 97 zeros, 1, 158 zeros, 1, and the 0
    b = Bits()
    dynamic_block(b, {97: 1, 256: 1}, {}, [97] * 40, cl_lens={18: 1, 0: 2, 1: 2},
                  sequence=[(18, 97 - 11), 1, (18, 138 - 11), (18, 20 - 11), 1, 0])
    out["hdist_1_no_distance_code"] = (zlib_wrap(b, b"a" * 40), b"a" * 40)
    # one distance code of one bit, as this project's encoder declares it
    b = Bits()
    dynamic_block(b, {97: 2, 98: 2, 256: 2, 257: 2}, {0: 1}, [97, 98, (3, 1), 97])
    out["single_distance_code"] = (zlib_wrap(b, b"abbbba"), b"abbbba")
    # repeats: 16 after a length, 17 and 18 for zeros
    b = Bits()
    lens = {s: 8 for s in range(256)}
    lens[256] = 8  # 257 codes of 8 bits over-subscribe: 255 of 8, two of 9
    lens[255] = lens[256] = 9
    seq = [8, (16, 3), (16, 3)] + [8] * (255 - 13) + [9, 9] + [0]
    cl = {**{s: 4 for s in range(14)}, 14: 5, 15: 5, 16: 5, 17: 5}
    dynamic_block(b, lens, {}, list(range(0, 256, 5)), cl_lens=cl, sequence=seq)
    out["repeat_16"] = (zlib_wrap(b, bytes(range(0, 256, 5))), bytes(range(0, 256, 5)))
    # empty blocks: an empty stored one, an empty fixed one, then data; and a payload of nothing
    b = Bits()
    stored_block(b, b"")
    fixed_block(b, [], final=False)
    fixed_block(b, [120, 121])
    out["empty_blocks"] = (zlib_wrap(b, b"xy"), b"xy")
    b = Bits()
    fixed_block(b, [])
    out["nothing"] = (zlib_wrap(b, b""), b"")
    # a literal/length code of the end-of-block symbol alone, one bit: incomplete, and taken
    b = Bits()
    dynamic_block(b, {256: 1}, {}, [])
    out["single_literal_code"] = (zlib_wrap(b, b""), b"")
    for name, (z, data) in out.items():
        assert inflate_by_zlib(z) == (data, True), name
    return out


@functools.lru_cache(None)
def refusals():
    """{name: (stream, expect)}: one per rule of csrc/inflate_rules.hpp.  zlib refuses each of them too, but for the ones that
    are whole streams of another size."""
    good = b"hello, hello, hello, hello"
    z = zlib.compress(good, 6)
    out = {"cm_not_8": (bytes([0x79, 0x9C ^ 0]) + z[2:], len(good)), "fdict": (bytes([0x78, 0xBB]) + z[2:], len(good)),
           "fcheck": (bytes([0x78, 0x9D]) + z[2:], len(good)), "cinfo_8": (bytes([0x88, 0x1C]) + z[2:], len(good)),
           "wrong_adler": (z[:-1] + bytes([z[-1] ^ 1]), len(good)), "byte_behind_the_adler": (z + b"\0", len(good)),
           "shorter_than_expect": (z, len(good) + 1), "longer_than_expect": (z, len(good) - 1), "no_stream": (b"", 4),
           "five_bytes": (z[:5], len(good))}
    assert (0x88 << 8 | 0x1C) % 31 == 0 and (0x78 << 8 | 0xBB) % 31 == 0 and (0x79 << 8 | 0x9C) % 31 != 0
    out["cm_not_8"] = (bytes([0x79, 0x9C + (31 - (0x799C % 31)) % 31]) + z[2:], len(good))

    def case(name, build, data=b"", expect=None):
        b = Bits()
        build(b)
        out[name] = (zlib_wrap(b, data), len(data) if expect is None else expect)

    case("block_type_3", lambda b: (b.put(1, 1), b.put(3, 2)))
    case("stored_nlen", lambda b: stored_block(b, b"abc", final=True, nlen=0x1234), b"abc")
    case("no_final_block", lambda b: fixed_block(b, [97], final=False), b"a")
    case("oversubscribed_literal_code", lambda b: dynamic_block(b, {97: 1, 98: 1, 256: 1}, {}, [97]), b"a")
    case("incomplete_literal_code", lambda b: dynamic_block(b, {97: 2, 256: 2}, {}, [97]), b"a")
    case("single_literal_code_of_two_bits", lambda b: dynamic_block(b, {256: 2}, {}, []))
    case("incomplete_distance_code", lambda b: dynamic_block(b, {97: 1, 256: 2, 257: 2}, {0: 2}, [97]), b"a")
    case("two_distance_codes_of_two_bits", lambda b: dynamic_block(b, {97: 1, 256: 2, 257: 2}, {0: 2, 1: 2}, [97]), b"a")
    case("oversubscribed_distance_code", lambda b: dynamic_block(b, {97: 1, 256: 2, 257: 2}, {0: 1, 1: 1, 2: 1}, [97]), b"a")
    case("no_end_of_block_code", lambda b: dynamic_block(b, {97: 1, 98: 1}, {}, [97], eob=False), b"a")
    case("oversubscribed_code_length_code", lambda b: dynamic_block(b, {97: 1, 256: 1}, {}, [97], cl_lens={0: 1, 1: 1, 2: 1}), b"a")
    case("incomplete_code_length_code", lambda b: dynamic_block(b, {97: 1, 256: 1}, {}, [97], cl_lens={0: 2, 1: 2}), b"a")
    case("hlit_287", lambda b: dynamic_block(b, {97: 1, 256: 1}, {}, [97], hlit=287), b"a")
    case("hdist_31", lambda b: dynamic_block(b, {97: 1, 256: 1}, {}, [97], hdist=31), b"a")
    case("repeat_with_nothing_before", lambda b: dynamic_block(b, {97: 1, 256: 1}, {}, [97], cl_lens=CL_WITH_16,
                                                               sequence=[(16, 0)] + [0] * 254 + [1, 0]), b"a")
    case("repeat_beyond_the_lengths", lambda b: dynamic_block(b, {97: 1, 256: 1}, {}, [97], cl_lens=CL_WITH_16,
                                                              sequence=[0] * 97 + [1] + [0] * 158 + [1, (16, 3)]), b"a")
    case("symbol_286", lambda b: fixed_block(b, [97, ("sym", 286)]), b"a")
    case("distance_symbol_30", lambda b: fixed_block(b, [97, 98, 99, ("dsym", 3, 30)]), b"abcabc")
    case("distance_beyond_the_output", lambda b: fixed_block(b, [97, 98, (3, 3)]), b"ababa")
    case("match_beyond_expect", lambda b: fixed_block(b, [97, (258, 1)]), b"a" * 259, expect=200)
    case("literal_beyond_expect", lambda b: fixed_block(b, [97, 98, 99]), b"abc", expect=2)
    case("stored_beyond_expect", lambda b: stored_block(b, b"abcdef", final=True), b"abcdef", expect=5)
    case("stored_beyond_the_stream", lambda b: (b.put(1, 1), b.put(0, 2), b.align(), b.put(500, 16), b.put(500 ^ 0xFFFF, 16)), b"")
    for name, (s, expect) in out.items():
        data, ok = inflate_by_zlib(s)
        assert not ok or len(data) != expect, name
    return out


@functools.lru_cache(None)
def small_stream():
    """a stream with a stored, a fixed and a dynamic block, for truncation at every byte"""
    data = payload("text", 700) + payload("noise", 90) + payload("zeros", 400)
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 9)
    z = c.compress(data[:700]) + c.flush(zlib.Z_FULL_FLUSH)
    c2 = zlib.compressobj(0, zlib.DEFLATED, -15)
    c3 = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_FIXED)
    z += c2.compress(data[700:790]) + c2.flush(zlib.Z_FULL_FLUSH) + c3.compress(data[790:]) + c3.flush()
    z += struct.pack(">I", zlib.adler32(data))
    assert inflate_by_zlib(z) == (data, True)
    return z, data


def mutations(z, count, seed):
    """count copies of z with one to three bytes changed"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        m = bytearray(z)
        for _ in range(int(rng.integers(1, 4))):
            m[int(rng.integers(0, len(m)))] ^= int(rng.integers(1, 256))
        out.append(bytes(m))
    return out


@functools.lru_cache(None)
def zoo(sizes=SIZES):
    """[(name, stream, payload)]: every well-formed stream of the tests but this project's own"""
    out = []
    for n in sizes:
        for kind in KINDS:
            data = payload(kind, n)
            for name, kw in VARIANTS:
                out.append((f"{kind}_{n}_{name}", deflate(data, **kw), data))
    out += [(name, z, data) for name, (z, data) in hand_cases().items()]
    return out


# ---- the TIFF builder ------------------------------------------------------------------------------------------------------------
def raster(layout, h, w, seed=5):
    """a raster with structure and noise: layout 1, 3, 4 (uint8 samples) or "f" (float32 with NaNs)"""
    rng = np.random.default_rng(seed + h * 31 + w)
    y, x = np.mgrid[0:h, 0:w]
    if layout == "f":
        a = (50 + 0.1 * x + 0.05 * y + rng.normal(0, 0.01, (h, w))).astype(np.float32)
        a[h // 3:h // 3 + 2, : w // 2] = np.nan
        return a
    base = (x * 3 + y * 5)[..., None] + np.arange(layout)[None, None, :] * 40 + rng.integers(0, 4, (h, w, layout))
    return (base & 255).astype(np.uint8)


def predicted_tile(tile, predictor):
    """the bytes a TIFF writer deflates for a tile: (th, tw, s) uint8 or (th, tw) float32"""
    if predictor == 1:
        return tile.tobytes()
    t = tile.view(np.uint32) if tile.dtype == np.float32 else tile
    d = t.copy()
    d[:, 1:] = t[:, 1:] - t[:, :-1]
    return d.tobytes()


def build_tiff(levels, tile=(512, 512), big=False, predictor=2, compression=8, level=6, sparse=False, geo=None, nodata=None,
               override=None, drop=(), byte_order=b"II", next_of_last=0, threads=1):
    """A tiled DEFLATE TIFF as bytes: levels - one array or a list, the full raster first - of (h, w, s) uint8 or (h, w)
    float32.  threads: the tiles of a tile row are deflated by that many threads.  override: {tag: (type, values)} replaces or adds tags of every IFD; drop: tags left out; next_of_last: where the
    last IFD's link points (an IFD loop)."""
    levels = levels if isinstance(levels, (list, tuple)) else [levels]
    tw, th = tile
    out = bytearray(byte_order + (b"+\0\x08\0\0\0" + bytes(8) if big else b"*\0" + bytes(4)))
    link, inline = (8, 8) if big else (4, 4)
    fmt_off = "<Q" if big else "<I"
    ifd_offsets = []

    def put(data):
        if len(out) & 1:
            out.append(0)
        at = len(out)
        out.extend(data)
        return at

    for index, a in enumerate(levels):
        is_float = a.dtype == np.float32
        h, w = a.shape[:2]
        s = 1 if is_float else a.shape[2]
        offs, cnts = [], []
        def stream(ty, tx):
            t = np.zeros((th, tw) + a.shape[2:], a.dtype)
            part = a[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw]
            t[:part.shape[0], :part.shape[1]] = part
            if sparse and not t.view(np.uint8).any():
                return b""
            return zlib.compress(predicted_tile(t, predictor), level)

        for ty in range(-(-h // th)):
            cols = range(-(-w // tw))
            if threads > 1:  # zlib releases the interpreter lock: the measurement script's large files
                from concurrent.futures import ThreadPoolExecutor

                with ThreadPoolExecutor(threads) as pool:
                    row = list(pool.map(lambda tx: stream(ty, tx), cols))
            else:
                row = [stream(ty, tx) for tx in cols]
            for z in row:
                offs.append(put(z) if z else 0), cnts.append(len(z))
        S, L, D, A, L8 = 3, 4, 12, 2, 16
        tags = {256: (L, [w]), 257: (L, [h]), 258: (S, [32] if is_float else [8] * s), 259: (S, [compression]),
                262: (S, [1 if s < 3 else 2]), 277: (S, [s]), 284: (S, [1]), 317: (S, [predictor]), 322: (S, [tw]), 323: (S, [th]),
                324: (L8 if big else L, offs), 325: (L, cnts), 339: (S, [3] if is_float else [1] * s)}
        if s == 4:
            tags[338] = (S, [2])
        if index:
            tags[254] = (L, [1])
        elif geo is not None:
            keys = [(1024, 0, 1, 1), (1025, 0, 1, 1), (3072, 0, 1, int(geo["epsg"]))] if geo.get("epsg") is not None else [(1025, 0, 1, 1)]
            tags[33550] = (D, [geo.get("gsd_x", geo.get("gsd")), geo.get("gsd_y", geo.get("gsd")), 0.0])
            tags[33922] = (D, [0.0, 0.0, 0.0, geo["min_x"], geo["max_y"], 0.0])
            tags[34735] = (S, [1, 1, 0, len(keys)] + [v for k in keys for v in k])
        if nodata is not None:
            tags[42113] = (A, nodata.encode() + b"\0")
        tags.update(override or {})
        for t in drop:
            tags.pop(t, None)
        dtypes = {S: "<u2", L: "<u4", D: "<f8", L8: "<u8"}
        entries = []
        for tag in sorted(tags):
            typ, values = tags[tag]
            data = bytes(values) if typ == A else np.asarray(values).astype(dtypes[typ]).tobytes()
            field = data.ljust(inline, b"\0") if len(data) <= inline else struct.pack(fmt_off, put(data))
            entries.append(struct.pack("<HH", tag, typ) + struct.pack(fmt_off, len(values)) + field)
        at = put(struct.pack("<Q" if big else "<H", len(entries)) + b"".join(entries) + bytes(inline))
        out[link:link + inline] = struct.pack(fmt_off, at)
        link = len(out) - inline
        ifd_offsets.append(at)
    if next_of_last:
        out[link:link + inline] = struct.pack(fmt_off, ifd_offsets[0] if next_of_last is True else next_of_last)
    return bytes(out)


# ---- the stand-alone program under the sanitizers ---------------------------------------------------------------------------
@functools.lru_cache(None)
def driver():
    """tests/geotiff_read_driver.cpp over the host route, built once per process with the address and undefined-behaviour
    sanitizers; without them where their runtime does not link.  Returns (path, sanitized)."""
    import os
    import subprocess
    import tempfile

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(tempfile.mkdtemp(prefix="geotiff_read_driver_"), "geotiff_read_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fopenmp", "-DOCHIP_GEOTIFF_READ_STANDALONE", "-I", os.path.join(root, "include"),
           "-o", exe, os.path.join(root, "tests", "geotiff_read_driver.cpp"),
           os.path.join(root, "opencalibration_amd", "csrc", "host", "geotiff_read.cpp")]
    if subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode == 0:
        return exe, True
    subprocess.run(cmd, check=True)
    return exe, False


def run_driver(jobs):
    """jobs: ("I", stream, expect) or ("R", layout tuple of 7, row0, rows, packed bytes, offsets uint64 array).  Returns per job
    (status, produced, payload or None) or (bad tile, raster bytes or None)."""
    import os
    import subprocess
    import tempfile

    exe, _ = driver()
    d = tempfile.mkdtemp(prefix="geotiff_read_run_")
    lines = []
    for i, job in enumerate(jobs):
        if job[0] == "I":
            with open(os.path.join(d, f"{i}.z"), "wb") as f:
                f.write(job[1])
            lines.append(f"I {os.path.join(d, f'{i}.z')} {int(job[2])} {os.path.join(d, f'{i}.out')}")
        else:
            with open(os.path.join(d, f"{i}.z"), "wb") as f:
                f.write(job[4])
            with open(os.path.join(d, f"{i}.off"), "wb") as f:
                f.write(np.ascontiguousarray(job[5], np.uint64).tobytes())
            lines.append("R " + " ".join(str(int(v)) for v in job[1]) + f" {int(job[2])} {int(job[3])} {os.path.join(d, f'{i}.z')} "
                         f"{os.path.join(d, f'{i}.off')} {os.path.join(d, f'{i}.out')}")
    with open(os.path.join(d, "list.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, os.path.join(d, "list.txt")], capture_output=True, text=True, timeout=600,
                       env={**os.environ, "OMP_NUM_THREADS": "4"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rows = r.stdout.strip().splitlines()
    assert len(rows) == len(jobs), r.stdout[-2000:]
    out = []
    for i, (row, job) in enumerate(zip(rows, jobs)):
        path = os.path.join(d, f"{i}.out")
        data = open(path, "rb").read() if os.path.exists(path) else None
        if job[0] == "I":
            status, produced = row.split()
            out.append((int(status), int(produced), data))
        else:
            out.append((int(row), data))
    return out
