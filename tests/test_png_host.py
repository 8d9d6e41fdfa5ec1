"""The PNG codec on the CPU route (csrc/png_rules.hpp, csrc/host/png.cpp, csrc/host/png_decode.hpp).
The encoder's files are read by Pillow and taken apart with zlib: pixels, payload, chunk CRCs, the size bound.  The decoder
reads files Pillow and the test's own writer produce and refuses what it does not take; truncated and mutated files are
corrupt or decode to Pillow's pixels.  Then base64, the graph's thumbnails through graph.json, checkpoints, the tile updates
and the refusals.  Nothing loaded into Python runs under a sanitizer: the rules and the decoder are driven by a stand-alone
program (png_rules_driver.cpp) built with the system g++."""
import base64
import functools
import inspect
import io
import json
import os
import struct
import subprocess
import warnings
import zlib

import numpy as np
import pytest
from PIL import Image

import png_fixtures as F
from ortho_fixtures import DOWN, cloud_surface, make_graph
from thumbnail_fixtures import images as thumbnail_images
from tile_progress_fixtures import blended, layers, plan_of
from opencalibration_amd import capi, host

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(None)
def files(bgr):
    """every fixture's file, one batch per channel order"""
    with host.PngEncoder() as e:
        return dict(zip(F.ALL, e.encode([F.image(k) for k in F.ALL], bgr=bgr)))


def pillow(data):
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im)


# ---- the encoder's files ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("name", F.ALL)
def test_file(name, bgr):
    a, data = F.image(name), files(bgr)[name]
    want = F.swapped(a) if bgr else a
    assert np.array_equal(pillow(data), want)
    parts = F.chunks(data)
    assert [k for k, _, _, _ in parts] == [b"IHDR", b"IDAT", b"IEND"]  # one IDAT, no ancillary chunks
    for kind, body, crc, _ in parts:
        assert crc == zlib.crc32(kind + body), kind
    c = 1 if a.ndim == 2 else a.shape[2]
    assert parts[0][1] == F.ihdr(a.shape[1], a.shape[0], 8, {1: 0, 3: 2, 4: 6}[c])
    payload = host.png_filter(a, bgr=bgr)
    assert parts[1][1][:2] == b"\x78\x9c"
    assert zlib.decompress(parts[1][1]) == payload.tobytes()
    assert len(data) <= F.stored_bytes(F.payload_bytes(a)) + 57
    assert np.array_equal(host.decode_png(data), want)
    assert host.encode_png(a, bgr=bgr) == data  # one by one as in the batch


def test_noise_is_stored_at_exactly_the_bound():
    a = F.image("gray_noise_300")
    S = F.stored_bytes(300 * 301)
    assert S == 2 + 300 * 301 + 2 * 5 + 4
    data = files(False)["gray_noise_300"]
    assert len(data) == S + 57
    z = F.idat_of(data)
    assert z[2] == 0 and z[3:5] == b"\xff\xff" and z[2 + 5 + 65535] == 1  # two stored blocks, the second final


# ---- the filter ----------------------------------------------------------------------------------------------------------
def filter_restated(a):
    """The five filters and the choice in numpy: per row the type with the smallest sum of min(v, 256 - v), the lowest on a tie"""
    h = a.shape[0]
    c = 1 if a.ndim == 2 else a.shape[2]
    raw = a.reshape(h, -1).astype(np.int32)
    left = np.zeros_like(raw)
    left[:, c:] = raw[:, :-c]
    up = np.zeros_like(raw)
    up[1:] = raw[:-1]
    ul = np.zeros_like(raw)
    ul[1:, c:] = raw[:-1, :-c]
    p = left + up - ul
    pa, pb, pc = abs(p - left), abs(p - up), abs(p - ul)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    cand = np.stack([raw, raw - left, raw - up, raw - (left + up) // 2, raw - paeth]).astype(np.uint8)  # (5, h, n)
    cost = np.minimum(cand.astype(np.int64), 256 - cand.astype(np.int64)).sum(2)  # (5, h)
    best = np.argmin(cost, 0)  # the first minimum: the lowest type
    rows = cand[best, np.arange(h)]
    return np.concatenate([best[:, None].astype(np.uint8), rows], 1).reshape(-1)


@pytest.mark.parametrize("name", F.ALL)
def test_filter_equals_restatement(name):
    a = F.image(name)
    assert np.array_equal(host.png_filter(a), filter_restated(a))
    assert np.array_equal(host.png_filter(a, bgr=True), filter_restated(F.swapped(a)))


def test_every_filter_type_is_chosen_somewhere():
    used = set()
    for name in F.ALL:
        a = F.image(name)
        used |= set(host.png_filter(a).reshape(a.shape[0], -1)[:, 0].tolist())
    assert used == {0, 1, 2, 3, 4}


# ---- the size ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.COMPRESSIBLE_LARGE)
def test_size_against_huffman_only(name):
    """The block coder's bound of test_geotiff_host.py: at most 1.05 x zlib's Huffman-only stream of the same payload"""
    payload = host.png_filter(F.image(name)).tobytes()
    assert len(payload) >= 65536
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
    ref = len(co.compress(payload) + co.flush())
    got = len(F.idat_of(files(False)[name]))
    print(f"{name}: {got} bytes against {ref} Huffman-only, ratio {got / ref:.4f}")
    assert got <= 1.05 * ref


# ---- the decoder against the outside -----------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 2), (2, 1), (1, 7), (7, 1), (3, 5), (5, 3), (16, 16), (17, 31), (43, 58), (64, 1), (1, 300), (300, 1),
          (100, 257), (129, 127), (200, 333), (256, 512)]
MODES = {"L": 1, "LA": 2, "RGB": 3, "RGBA": 4}


def picture(h, w, c, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([(x * (k + 2) + y * (5 - k) + rng.integers(0, 3, (h, w))) & 255 for k in range(c)], -1).astype(np.uint8)
    return a[..., 0] if c == 1 else a


def pillow_file(a, mode, **kw):
    f = io.BytesIO()
    im = a if isinstance(a, Image.Image) else Image.fromarray(a)
    assert im.mode == mode
    im.save(f, "PNG", **kw)
    return f.getvalue()


def decoded_as_pillow(data):
    want = pillow(data)
    got = host.decode_png(data)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_decoder_reads_pillow_files():
    assert len(SHAPES) == 17
    for i, (h, w) in enumerate(SHAPES):
        for mode, c in MODES.items():
            a = picture(h, w, c, 100 * i + c)
            for kw in (dict(compress_level=0), dict(compress_level=1), dict(compress_level=9), dict(optimize=True)):
                data = pillow_file(a, mode, **kw)
                info = host.png_info(data)
                assert (info["width"], info["height"], info["channels"], info["status"]) == (w, h, c, host.PNG_OK)
                got = host.decode_png(data)
                assert np.array_equal(got, a), (h, w, mode, kw)


def test_decoder_split_idats_and_ancillary_chunks():
    a = picture(129, 127, 3, 9)
    data = pillow_file(a, "RGB", compress_level=6)
    parts = [(k, b) for k, b, _, _ in F.chunks(data)]
    z = F.idat_of(data)
    for step in (1, 7, 1000, len(z)):
        split = [(b"IDAT", z[i:i + step]) for i in range(0, len(z), step)] + [(b"IDAT", b"")]
        out = F.rebuilt([parts[0], (b"tEXt", b"Comment\x00split"), (b"pHYs", struct.pack(">IIB", 2835, 2835, 1))] + split
                        + [(b"tIME", bytes(7)), (b"IEND", b"")])
        assert np.array_equal(host.decode_png(out), a), step
        decoded_as_pillow(out)
    # an IDAT behind another chunk is no continuation
    broken = F.rebuilt([parts[0], (b"IDAT", z[:50]), (b"tEXt", b"a\x00b"), (b"IDAT", z[50:]), (b"IEND", b"")])
    with pytest.raises(host.PngError) as e:
        host.decode_png(broken)
    assert e.value.status == host.PNG_CORRUPT


def own_file(a, kind, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15):
    """rows of one forced filter type each, the filter and zlib done here"""
    h = a.shape[0]
    c = 1 if a.ndim == 2 else a.shape[2]
    raw = a.reshape(h, -1).astype(np.int32)
    left = np.zeros_like(raw)
    left[:, c:] = raw[:, :-c]
    up = np.zeros_like(raw)
    up[1:] = raw[:-1]
    ul = np.zeros_like(raw)
    ul[1:, c:] = raw[:-1, :-c]
    p = left + up - ul
    pa, pb, pc = abs(p - left), abs(p - up), abs(p - ul)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    cand = np.stack([raw, raw - left, raw - up, raw - (left + up) // 2, raw - paeth]).astype(np.uint8)
    types = np.full(h, kind) if kind is not None else np.arange(h) % 5
    payload = np.concatenate([types[:, None].astype(np.uint8), cand[types, np.arange(h)]], 1).tobytes()
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    z = co.compress(payload) + co.flush()
    return F.rebuilt([(b"IHDR", F.ihdr(a.shape[1], h, 8, {1: 0, 2: 4, 3: 2, 4: 6}[c])), (b"IDAT", z), (b"IEND", b"")]), payload


def test_decoder_every_filter_type_and_block_kind():
    for c in (1, 2, 3, 4):
        a = picture(37, 53, c, 40 + c)
        for kind in (0, 1, 2, 3, 4, None):
            data, _ = own_file(a, kind)
            assert np.array_equal(host.decode_png(data), a), (c, kind)
            decoded_as_pillow(data)
    a = picture(200, 333, 3, 77)
    for kw in (dict(level=0), dict(strategy=zlib.Z_FIXED), dict(strategy=zlib.Z_HUFFMAN_ONLY), dict(strategy=zlib.Z_RLE), dict(level=9),
               dict(wbits=9), dict(level=9, wbits=15)):
        data, _ = own_file(a, None, **kw)
        assert np.array_equal(host.decode_png(data), a), kw
    # a long-distance match: the second half repeats the first 32 768 bytes back
    rng = np.random.default_rng(3)
    half = rng.integers(0, 256, (32, 1023), dtype=np.uint8)  # 32 rows of 1 + 1 023 bytes: 32 768
    data, _ = own_file(np.concatenate([half, half]), 0, level=9)
    assert np.array_equal(host.decode_png(data), np.concatenate([half, half]))


def status_of(data):
    try:
        host.decode_png(data)
    except host.PngError as e:
        return e.status
    return host.PNG_OK


def test_decoder_unsupported():
    a = picture(20, 30, 3, 5)
    palette = pillow_file(Image.fromarray(a).quantize(16), "P")
    sixteen = pillow_file((picture(20, 30, 1, 6).astype(np.uint16) * 257), "I;16")
    one_bit = pillow_file(picture(20, 30, 1, 7) > 127, "1")
    data, _ = own_file(a, 1)
    parts = [(k, b) for k, b, _, _ in F.chunks(data)]
    interlaced = F.rebuilt([(b"IHDR", F.ihdr(30, 20, 8, 2, 1))] + parts[1:])
    for name, f in (("palette", palette), ("16-bit", sixteen), ("1-bit", one_bit), ("interlaced", interlaced)):
        assert host.png_info(f)["status"] == host.PNG_UNSUPPORTED, name
        assert status_of(f) == host.PNG_UNSUPPORTED, name


def test_decoder_corrupt_structures():
    a = picture(20, 30, 3, 5)
    data, payload = own_file(a, None)
    parts = [(k, b) for k, b, _, _ in F.chunks(data)]
    z = parts[1][1]
    cases = dict(
        trailing_garbage_in_stream=F.rebuilt([parts[0], (b"IDAT", z + b"\x00"), parts[2]]),
        trailing_garbage_after_iend=data + b"\x00",
        short_stream=F.rebuilt([parts[0], (b"IDAT", zlib.compress(payload[:-1])), parts[2]]),
        long_stream=F.rebuilt([parts[0], (b"IDAT", zlib.compress(payload + b"\x00")), parts[2]]),
        filter_type_5=F.rebuilt([parts[0], (b"IDAT", zlib.compress(b"\x05" + payload[1:])), parts[2]]),
        bad_adler=F.rebuilt([parts[0], (b"IDAT", z[:-1] + bytes([z[-1] ^ 1])), parts[2]]),
        no_idat=F.rebuilt([parts[0], parts[2]]),
        no_iend=F.rebuilt(parts[:2]),
        bad_crc=data[:-1] + bytes([data[-1] ^ 1]),
        unknown_critical=F.rebuilt([parts[0], (b"ABCD", b""), parts[1], parts[2]]),
        zero_width=F.rebuilt([(b"IHDR", F.ihdr(0, 20, 8, 2))] + parts[1:]),
        depth_3=F.rebuilt([(b"IHDR", F.ihdr(30, 20, 3, 2))] + parts[1:]),
        preset_dictionary=F.rebuilt([parts[0], (b"IDAT", b"\x78\xbb" + z[2:]), parts[2]]),
        not_a_png=b"GIF89a" + data[6:],
    )
    for name, f in cases.items():
        assert status_of(f) == host.PNG_CORRUPT, name
    assert status_of(data) == host.PNG_OK


def test_truncations_and_mutations():
    """Corrupt, or exactly Pillow's pixels; never a third answer.  Pillow may itself refuse a file this decoder takes or
    tolerate one it refuses (a damaged IEND): only the cases where both decode are compared."""
    data = files(False)["thumb_noisy"]
    ok = F.image("thumb_noisy")
    parts = F.chunks(data)
    cuts = sorted({at for _, _, _, at in parts} | {at + 4 for _, _, _, at in parts} | {at + 8 for _, _, _, at in parts}
                  | {len(data) - 4, len(data) - 1, 0, 1, 8})
    for cut in cuts:
        assert status_of(data[:cut]) == host.PNG_CORRUPT, cut
    rng = np.random.default_rng(99)
    both = differ = skipped = corrupt = 0
    for k in range(600):
        m = bytearray(data)
        at = int(rng.integers(0, len(m))) if k >= len(parts) * 12 else None
        if at is None:  # first every byte of the chunks' lengths, types and CRCs in turn
            _, body, _, start = parts[k // 12]
            j = k % 12
            at = start + j if j < 8 else start + 8 + len(body) + (j - 8)
        m[at] ^= 1 << int(rng.integers(0, 8))
        m = bytes(m)
        try:
            got = host.decode_png(m)
        except host.PngError as e:
            assert e.status == host.PNG_CORRUPT, at  # the IHDR's CRC is checked before its depth and type are looked at
            corrupt += 1
            continue
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                want = pillow(m)
        except Exception:
            skipped += 1
            continue
        both += 1
        differ += int(got.shape != want.shape or not np.array_equal(got, want))
    print(f"600 mutations: {corrupt} refused, {both} decoded by both, {skipped} decoded here and refused by Pillow")
    assert differ == 0
    assert corrupt > 500  # a CRC guards every byte but the IEND's own
    assert np.array_equal(host.decode_png(data), ok)


# ---- base64 ----------------------------------------------------------------------------------------------------------------
def test_base64():
    names = ("one_gray", "one_rgb", "one_rgba", "five_by_three", "thumb_noisy", "gray_noise_300")
    with host.PngEncoder() as e:
        text = e.encode([F.image(k) for k in names], base64=True)
    lengths = set()
    for k, t in zip(names, text):
        assert isinstance(t, str) and t == base64.b64encode(files(False)[k]).decode()
        lengths.add(len(files(False)[k]) % 3)
    assert lengths == {0, 1, 2}  # no padding, one and two characters of it


# ---- the graph -------------------------------------------------------------------------------------------------------------
def preview_scene():
    pos, ori, model = [(0, 0, 10), (10, 0, 10)], [DOWN, DOWN], [500, 90, 62.5, 0, 0, 0, 0, 0, 180, 125]
    surface = [host.rebuild_mesh(np.array(pos, np.float64),
                                 previous=cloud_surface([(-2, -2, 0), (12, -2, 0), (12, 2, 0), (-2, 2, 0), (5, 0, 0)]))]
    views = thumbnail_images("integer_180x125")[:1].repeat(2, 0).copy()
    views[1] = 255 - views[1]
    return pos, ori, model, surface, views


def test_graph_thumbnails_through_json():
    pos, ori, model, surface, views = preview_scene()
    g = make_graph(pos, ori, model)
    g.make_thumbnails(views, g.node_ids)  # the load stage's thumbnails, CPU route
    pixels, ids = [g.thumbnail(i) for i in range(2)], list(g.node_ids)
    assert g.encode_thumbnails() == 2
    text = g.to_json()
    want = host.orthomosaic_thumbnail(g, surface)
    g.close()
    doc = json.loads(text)
    thumbs = [n["payload"]["thumbnail"] if "payload" in n else n["thumbnail"] for n in _nodes(doc)]
    for t, p in zip(thumbs, pixels):
        f = base64.b64decode(t)
        assert F.chunks(f)[0][1][9] == 2 and np.array_equal(pillow(f), p)  # colour type 2, the three bytes as stored
    g2 = host.Graph().from_json(text)
    with pytest.raises(capi.OchipError, match="thumbnail"):
        host.orthomosaic_thumbnail(g2, surface)
    assert g2.decode_thumbnails() == [host.PNG_OK, host.PNG_OK]
    for i, nid in enumerate(ids):  # a loaded graph orders its nodes by id
        assert np.array_equal(g2.thumbnail(g2.node_ids.index(nid)), pixels[i])
    got = host.orthomosaic_thumbnail(g2, surface)
    assert g2.to_json() == text  # decoding leaves the text as it was
    g2.close()
    assert np.array_equal(got["rgba"], want["rgba"]) and np.array_equal(got["ids"], want["ids"])


def _nodes(doc):
    """the node records of a graph.json document, wherever this version keeps them"""
    found = []

    def walk(v):
        if isinstance(v, dict):
            if "thumbnail" in v:
                found.append(v)
            for x in v.values():
                walk(x)
        elif isinstance(v, list):
            for x in v:
                walk(x)

    walk(doc)
    return found


def with_thumbnails(text, thumbs):
    doc = json.loads(text)
    nodes = _nodes(doc)
    assert len(nodes) == len(thumbs)
    for n, t in zip(nodes, thumbs):
        n["thumbnail"] = t
    return json.dumps(doc)


def test_graph_json_with_pillow_thumbnails():
    pos, ori, model, surface, _ = preview_scene()
    pos, ori = pos + [(5, 0, 10), (5, 1, 10)], ori + [DOWN, DOWN]
    g = make_graph(pos, ori, model)
    text = g.to_json()
    g.close()
    rgb, gray, rgba = picture(42, 60, 3, 1), picture(42, 60, 1, 2), picture(42, 60, 4, 3)
    thumbs = [base64.b64encode(pillow_file(rgb, "RGB")).decode(), base64.b64encode(pillow_file(gray, "L")).decode(),
              base64.b64encode(pillow_file(rgba, "RGBA")).decode(),
              base64.b64encode(pillow_file(Image.fromarray(rgb).quantize(8), "P")).decode()]
    g = host.Graph().from_json(with_thumbnails(text, thumbs))
    found = [n["thumbnail"] for n in _nodes(json.loads(g.to_json()))]
    status = g.decode_thumbnails()
    by_text = dict(zip(found, status))
    assert [by_text[t] for t in thumbs] == [host.PNG_OK, host.PNG_OK, host.PNG_OK, host.PNG_UNSUPPORTED]
    pictures = {thumbs[0]: rgb, thumbs[1]: np.repeat(gray[..., None], 3, 2), thumbs[2]: rgba[..., :3], thumbs[3]: None}
    for i, t in enumerate(found):
        got = g.thumbnail(i)
        if pictures[t] is None:
            assert got is None  # the refused node is left as it was: bare
        else:
            assert np.array_equal(got, pictures[t])
    # a refused thumbnail leaves an earlier decoded one alone as well
    idx = found.index(thumbs[0])
    g.set_thumbnail(idx, rgb[::-1].copy())
    g2_text = with_thumbnails(g.to_json(), ["AAAA" if t == thumbs[0] else t for t in found])
    g.close()
    g3 = host.Graph().from_json(g2_text)
    g3.set_thumbnail(idx, rgb[::-1].copy())
    st = g3.decode_thumbnails()
    assert st[idx] == host.PNG_CORRUPT and np.array_equal(g3.thumbnail(idx), rgb[::-1])
    g3.close()


def test_checkpoint_defaults_and_thumbnails(tmp_path):
    for fn, names in ((host.save_checkpoint, ("encode_thumbnails", "ctx")), (host.load_checkpoint, ("decode_thumbnails",))):
        for n in names:
            assert inspect.signature(fn).parameters[n].default in (False, None)
    pos, ori, model, surface, views = preview_scene()
    g = make_graph(pos, ori, model)
    g.make_thumbnails(views, g.node_ids)
    want = host.orthomosaic_thumbnail(g, surface)
    host.save_checkpoint(tmp_path / "plain", g, surface)
    # the default's files against the ones the commit before this codec wrote for this scene (tests/golden/png/parent_checkpoint)
    recorded = os.path.join(HERE, "golden", "png", "parent_checkpoint")
    assert sorted(os.listdir(recorded)) == sorted(os.listdir(tmp_path / "plain")) and len(os.listdir(recorded)) == 4
    for name in os.listdir(recorded):
        with open(os.path.join(recorded, name), "rb") as f:
            assert (tmp_path / "plain" / name).read_bytes() == f.read(), name
    g0, s0, meta0 = host.load_checkpoint(recorded)  # and the default load of them: no thumbnails, the preview refuses
    assert g0.thumbnail(0) is None and len(s0) == 1 and meta0["state"] == "INITIAL_PROCESSING"
    with pytest.raises(capi.OchipError, match="thumbnail"):
        host.orthomosaic_thumbnail(g0, s0)
    g0.close()
    plain = (tmp_path / "plain" / "graph.json").read_bytes()
    assert all(n["thumbnail"] == "" for n in _nodes(json.loads(plain)))  # the default: as before, no thumbnail text
    host.save_checkpoint(tmp_path / "thumbs", g, surface, encode_thumbnails=True)
    g.close()
    g1, s1, _ = host.load_checkpoint(tmp_path / "thumbs")
    assert g1.thumbnail(0) is None  # the default: the text is carried, nothing is decoded
    host.save_checkpoint(tmp_path / "again", g1, s1)
    assert (tmp_path / "again" / "graph.json").read_bytes() == (tmp_path / "thumbs" / "graph.json").read_bytes()
    g1.close()
    g2, s2, _ = host.load_checkpoint(tmp_path / "thumbs", decode_thumbnails=True)
    got = host.orthomosaic_thumbnail(g2, s2)
    g2.close()
    assert np.array_equal(got["rgba"], want["rgba"])


# ---- the tile updates ------------------------------------------------------------------------------------------------------
def test_tile_progress_png():
    cols, rows, t = 300, 130, 128
    plan = plan_of(cols, rows)
    bgra, weight = layers("mixed", 2, rows, cols)
    with host.TileProgress(plan, t, 2) as p:
        p.feed(host.TILE_PASS_LAYERS, 0, bgra, weight)
        p.feed(host.TILE_PASS_BLEND, 0, blended("alpha_mixed", rows, cols))
        plain, with_png = p.collect(), p.collect(png=True)
    assert len(plain) == len(with_png) == 6 and all("png_base64" not in u for u in plain)
    for u in with_png:
        got = pillow(base64.b64decode(u["png_base64"]))
        assert np.array_equal(got, u["thumbnail"][..., [2, 1, 0, 3]])
    assert inspect.signature(host.ortho_mosaic).parameters["progress_png"].default is False
    assert inspect.signature(host.ortho_mosaic_streamed).parameters["progress_png"].default is False


# ---- the refusals ----------------------------------------------------------------------------------------------------------
def test_encoder_refusals():
    ok = F.image("five_by_three")
    with host.PngEncoder() as e:
        for bad in (ok.astype(np.uint16), ok.astype(np.float32), np.zeros((4, 4, 2), np.uint8), np.zeros((4, 4, 5), np.uint8),
                    np.zeros((0, 4, 3), np.uint8), np.zeros((4, 0), np.uint8), np.zeros((2, 2, 2, 3), np.uint8)):
            with pytest.raises(ValueError):
                e.encode([ok, bad])
        with pytest.raises(ValueError, match="65535"):
            e.encode([F.image("one_gray")] * 65536)
        with pytest.raises(capi.OchipError, match="add up to"):
            e.encode([ok, ok], cap=2 * (F.stored_bytes(F.payload_bytes(ok)) + 57) - 1)
        assert e.encode([]) == []
        # through the entry point itself: channels, sizes, the batch limit, NULL arrays - nothing is written
        L = host.load()
        out, offsets = np.full(4096, 0xAB, np.uint8), np.full(3, 7, np.uint64)
        px = np.zeros(64, np.uint8)

        def call(n, recs, out_ptr=out.ctypes.data, cap=out.size, off_ptr=offsets.ctypes.data, handle=None):
            arr = (capi.PngImage * max(len(recs), 1))(*[capi.PngImage(*r) for r in recs])
            return L.och_png_encoder_encode(e.h if handle is None else handle, n, arr if recs else None, 0, 0, out_ptr, cap, off_ptr)

        good = (px.ctypes.data, 4, 4, 3, 0)
        for n, recs in ((2, [good, (px.ctypes.data, 4, 4, 2, 0)]), (2, [good, (px.ctypes.data, 4, 4, 5, 0)]), (1, [(px.ctypes.data, 0, 4, 3, 0)]),
                        (1, [(px.ctypes.data, 4, 65536, 1, 0)]), (1, [(None, 4, 4, 3, 0)]), (65536, [good]), (-1, [good]), (1, []),
                        (1, [(px.ctypes.data, 65535, 65535, 1, 0)])):
            assert call(n, recs) != 0, (n, recs)
            assert L.och_png_last_error()
        assert call(1, [good], out_ptr=None) != 0 and call(1, [good], off_ptr=None) != 0 and call(1, [good], cap=10) != 0
        assert (out == 0xAB).all() and (offsets == 7).all()
        dead = host.PngEncoder()
        h = dead.h
        dead.close()
        assert call(1, [good], handle=h) != 0 and b"not a live" in L.och_png_last_error()
        assert call(1, [good]) == 0 and offsets[0] == 0 and offsets[1] > 57


def test_decoder_refusals():
    assert host.png_info(b"")["status"] == host.PNG_CORRUPT and host.png_info(None)["status"] == host.PNG_CORRUPT
    assert status_of(b"") == host.PNG_CORRUPT and status_of(None) == host.PNG_CORRUPT
    # 65 535 x 65 535 RGBA over a few bytes: the header is valid, the data cannot fill it, nothing is sized from it
    hostile = F.rebuilt([(b"IHDR", F.ihdr(65535, 65535, 8, 6)), (b"IDAT", zlib.compress(bytes(100))), (b"IEND", b"")])
    assert host.png_info(hostile)["status"] == host.PNG_OK
    assert status_of(hostile) == host.PNG_CORRUPT
    huge = F.rebuilt([(b"IHDR", F.ihdr(0x7FFFFFFF, 0x7FFFFFFF, 8, 6)), (b"IDAT", zlib.compress(bytes(100))), (b"IEND", b"")])
    assert status_of(huge) == host.PNG_CORRUPT


# ---- the rules and the decoder under the sanitizers ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("png_rules") / "driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-o", exe, os.path.join(HERE, "png_rules_driver.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:
        warnings.warn("the sanitizer runtimes do not link here: the driver runs plain")
        subprocess.run(cmd, check=True)
    return exe


def test_rules_under_sanitizers(driver):
    r = subprocess.run([driver], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "clean" in r.stdout
