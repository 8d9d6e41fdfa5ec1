"""The scenarios of test_gpu_jpeg_decode.py, run in a child process that brings torch up before libochip.so (as
jpeg_gpu_child.py does) and holds one capi.Context(0).  `python jpeg_decode_gpu_child.py <tests dir> <repo dir>` runs every
scenario and prints one JSON line {scenario: "ok" or the failure's traceback}.  A scenario that ends in a device error ends
the run: the ones after it are reported as not run.  The yardsticks are the CPU route of the same library (ctx None), which
test_jpeg_decode_host.py holds against libjpeg-turbo's pixels, and the committed pixels themselves."""
import json
import sys
import traceback

import numpy as np
import torch

torch.cuda.init()
if __name__ == "__main__":
    sys.path[:0] = sys.argv[1:3]

import jpeg_decode_fixtures as D  # noqa: E402
import jpeg_fixtures as F  # noqa: E402
from opencalibration_amd import capi, host  # noqa: E402

MIN_BITS, MIDDLE_BITS = 32, 256
# (name, content, height, width, subsequence_bits): this project's encoder writes them (4:2:0, quality 95).
#   noise 1024 x 1536: megabytes of scan, dozens of workgroups of 256 subsequences, several blocks of the scan
#   flat 16 x 4064 / 4080 / 4096 at 32 bits: 4 bytes an MCU, so 255, 256 and 257 subsequences - a workgroup less one, exact,
#     and one more (the child asserts the counts)
#   noise 16 x 1008 / 1024 / 1040: 63, 64 and 65 MCUs - the DC passes' chunk of 64 MCUs less one, exact, one more
#   ramp 16 x 80 / 96 / 256: 30, 36 and 96 blocks - the transform's 32 blocks a workgroup less two, over, and three exactly
#   ramp 16 x 16, 15 x 17, 1 x 257: 256, 255 and 257 pixels - the pixel kernel's workgroup
LARGE = [("noise_1024x1536", "noise", 1024, 1536, 0),
         ("flat_16x4064_255_subsequences", "flat", 16, 4064, MIN_BITS), ("flat_16x4080_256_subsequences", "flat", 16, 4080, MIN_BITS),
         ("flat_16x4096_257_subsequences", "flat", 16, 4096, MIN_BITS),
         ("noise_16x1008_63_mcus", "noise", 16, 1008, 0), ("noise_16x1024_64_mcus", "noise", 16, 1024, 0),
         ("noise_16x1040_65_mcus", "noise", 16, 1040, 0),
         ("ramp_16x80_30_blocks", "ramp", 16, 80, 0), ("ramp_16x96_36_blocks", "ramp", 16, 96, 0), ("ramp_16x256_96_blocks", "ramp", 16, 256, 0),
         ("ramp_16x16_256_pixels", "ramp", 16, 16, 0), ("ramp_15x17_255_pixels", "ramp", 15, 17, 0), ("ramp_1x257_257_pixels", "ramp", 1, 257, 0)]

_cpu = {}


def cpu_route(data, apply=True):
    """host.decode_jpeg on the CPU route: computed once per file, shared, left unchanged"""
    key = (data, apply)
    if key not in _cpu:
        _cpu[key] = host.decode_jpeg(data, apply_orientation=apply)
        _cpu[key].setflags(write=False)
    return _cpu[key]


def same(got, want, what):
    assert got.shape == want.shape, f"{what}: {got.shape} against {want.shape}"
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} samples differ, the first at {bad[0].tolist()}")


def scenario_fixtures(ctx, bits):
    names = sorted(D.golden_files())
    files = [D.golden_bytes(n) for n in names]
    with host.JpegDecoder(ctx, subsequence_bits=bits) as d:
        for apply in (True, False):
            b = d.decode(files, apply_orientation=apply)
            assert b.status == ["ok"] * len(files), b.status
            assert 1 <= b.rounds[0] and 1 <= b.rounds[1] <= 257, b.rounds
            pixels = b.pixels.cpu().numpy()
            for i, n in enumerate(names):
                h, w = b.shapes[i]
                got = pixels[b.offsets[i]:b.offsets[i] + h * w * 3].reshape(h, w, 3)
                same(got, cpu_route(files[i], apply), f"{n} in the batch, apply_orientation={apply}")
                D.check_golden(n, got, oriented=apply)
        for n, f in zip(names, files):
            b = d.decode([f])
            same(b.image(0).cpu().numpy(), cpu_route(f), f"{n} alone")


def scenario_large(ctx, case):
    name, kind, h, w, bits = case
    data = host.encode_jpeg(F.content(kind, h, w, 3))
    if bits:
        scan = len(data) - 2 - D.segments(data)[-1][1] - 14
        assert -(-scan * 8 // bits) == int(name.split("_")[2]), (name, scan)
    with host.JpegDecoder(ctx, subsequence_bits=bits) as d:
        b = d.decode([data])
        assert b.status == ["ok"]
        same(b.image(0).cpu().numpy(), cpu_route(data), name)
    if kind == "noise" and h > 1000:
        assert b.rounds[0] >= 2, b.rounds  # more than one workgroup: a launch to hand the states on, one to see them settled


def scenario_two_decoders(ctx):
    a, b = D.golden_bytes("noise_48x64_420_q100"), D.golden_bytes("sample_test2")
    with host.JpegDecoder(ctx) as da, host.JpegDecoder(ctx, subsequence_bits=64) as db:
        ra, rb = da.decode([a, b]), db.decode([b, a])
        rb2, ra2 = db.decode([a]), da.decode([b])
        same(ra.image(0).cpu().numpy(), cpu_route(a), "the first decoder, first file")
        same(ra.image(1).cpu().numpy(), cpu_route(b), "the first decoder, second file")
        same(rb.image(0).cpu().numpy(), cpu_route(b), "the second decoder, first file")
        same(rb.image(1).cpu().numpy(), cpu_route(a), "the second decoder, second file")
        same(rb2.image(0).cpu().numpy(), cpu_route(a), "the second decoder again")
        same(ra2.image(0).cpu().numpy(), cpu_route(b), "the first decoder again")


def scenario_unsupported_in_a_batch(ctx):
    good, gray = D.golden_bytes("noise_33x47_420"), D.golden_bytes("noise_33x47_gray")
    bad = D.unsupported_by_patch(D.golden_bytes("noise_33x47_444"), good)["arithmetic"]
    with host.JpegDecoder(ctx, subsequence_bits=MIN_BITS) as d:
        out = torch.full((3 * 33 * 47 * 3 + 64,), 201, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        b = d.decode([good, bad, gray, good], out=out)
    assert b.status == ["ok", "unsupported", "ok", "ok"] and b.shapes[1] is None and b.offsets == [0, None, 4653, 9306]
    same(b.image(0).cpu().numpy(), cpu_route(good), "ahead of the refused file")
    same(b.image(2).cpu().numpy(), cpu_route(gray), "behind the refused file")
    same(b.image(3).cpu().numpy(), cpu_route(good), "the last file")
    assert (out[3 * 33 * 47 * 3:] == 201).all()  # nothing written behind the last image
    with pytest_raises("unsupported"):
        host.decode_jpeg(bad, ctx=ctx)


def scenario_bytes_behind_the_last_block(ctx):
    """zero bytes between the scan and EOI decode as symbols of no block: both routes leave them unread"""
    for name in ("noise_33x47_420", "noise_33x47_gray", "noise_48x64_420_restart_1_row"):
        data = D.bytes_behind_the_last_block(D.golden_bytes(name))
        for bits in (MIN_BITS, 0):
            with host.JpegDecoder(ctx, subsequence_bits=bits) as d:
                b = d.decode([data])
            assert b.status == ["ok"], (name, bits, b.status)
            same(b.image(0).cpu().numpy(), cpu_route(data), f"{name} with bytes behind its last block, {bits} bits")
            D.check_golden(name, b.image(0).cpu().numpy())


def scenario_orientations(ctx):
    for name, o, _ in D.EXIF_GOLDEN[4:]:
        data = D.golden_bytes(name)
        got = host.decode_jpeg(data, ctx=ctx)
        assert got.shape == (40, 24, 3)
        same(got, cpu_route(data), name)
        D.check_golden(name, got)
        same(host.decode_jpeg(data, ctx=ctx, apply_orientation=False), cpu_route(data, False), name + " as stored")


class pytest_raises:
    def __init__(self, text):
        self.text = text

    def __enter__(self):
        return self

    def __exit__(self, kind, value, tb):
        assert kind is not None and issubclass(kind, (capi.OchipError, ValueError)), "not refused: " + self.text
        assert self.text in str(value), str(value)
        return True


def scenario_load_jpegs(ctx):
    """four small files of one size through Graph.load_jpegs against Graph.load_images of the host-decoded pixels"""
    h, w, f = 240, 320, 300.0
    rng = np.random.default_rng(12)
    y, x = np.mgrid[0:h, 0:w]
    files = []
    for i in range(4):
        img = np.zeros((h, w, 3), np.uint8)
        for _ in range(60):  # bright and dark discs on a gradient: corners for the detector
            cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(4, 20)
            img[(y - cy) ** 2 + (x - cx) ** 2 < r * r] = rng.integers(0, 256, 3)
        img = (img.astype(np.int32) // 2 + ((x + y + 13 * i) % 128)[..., None]).astype(np.uint8)
        files.append(host.encode_jpeg(img))
    pixels = np.stack([cpu_route(d) for d in files])
    model = np.array([f, w / 2, h / 2, 0, 0, 0, 0, 0, w, h], np.float64)
    pos = np.array([(i * 20.0, 3.0 * i, 100.0) for i in range(4)])
    g1, g2 = host.Graph(), host.Graph()
    m1 = g1.load_jpegs(ctx, files, g1.add_model(model), pos, max_keypoints=2000, thumbnails=True, chunk=3)
    m2 = g2.load_images(ctx, pixels, g2.add_model(model), pos, max_keypoints=2000, thumbnails=True)
    assert g1.num_nodes == g2.num_nodes == 4 and g1.node_ids == g2.node_ids
    assert np.allclose(m1, m2) and m2[0] > 0, (m1, m2)
    for i in range(4):
        a, b = g1.node_payload(i), g2.node_payload(i)
        for k in ("loc", "strength", "desc", "position"):
            assert np.array_equal(a[k], b[k]), (i, k)
    assert g1.to_json() == g2.to_json() and '"thumbnail"' in g1.to_json()
    bad = D.unsupported_by_patch(D.golden_bytes("noise_33x47_444"), D.golden_bytes("noise_33x47_420"))["twelve_bits"]
    with pytest_raises("file 1 is unsupported"):
        g1.load_jpegs(ctx, [files[0], bad], 0, pos[:2])
    with pytest_raises("47 x 33"):
        g1.load_jpegs(ctx, [files[0], D.golden_bytes("noise_33x47_420")], 0, pos[:2])
    g1.close(), g2.close()


def scenario_refusals(ctx):
    with pytest_raises("subsequence_bits 48"):
        host.JpegDecoder(ctx, subsequence_bits=48)
    with pytest_raises("subsequence_bits -32"):
        host.JpegDecoder(ctx, subsequence_bits=-32)
    good = D.golden_bytes("noise_33x47_420")
    with host.JpegDecoder(ctx) as d:
        small = torch.zeros(100, dtype=torch.uint8, device="cuda:0")
        with pytest_raises("the output holds 100"):
            d.decode([good], out=small)
        with pytest_raises("out must be"):
            d.decode([good], out=np.zeros(33 * 47 * 3, np.uint8))
        assert d.decode([]).status == []
        assert d.L.och_jpeg_decoder_decode(d.h, 65536, None, None, 1, None, 0, None, None, None) == -1
        assert "65536 files, at most 65535" in d._error()
        same(d.decode([good]).image(0).cpu().numpy(), cpu_route(good), "the decoder after its refusals")
        dead = d.h
    L = host.load()
    assert L.och_jpeg_decoder_decode(dead, 0, None, None, 1, None, 0, None, None, None) == -1  # a dead handle is refused, not followed
    assert "not a live" in L.och_jpeg_decode_last_error().decode()
    assert ctx.L.ochip_jpeg_decoder_decode(None, 0, None, None, 1, None, 0, None, None, None) == -1  # OCHIP_EINVAL
    ctx.L.ochip_jpeg_decoder_destroy(None)


def scenarios():
    s = dict(fixtures=(scenario_fixtures, 0), fixtures_smallest_subsequences=(scenario_fixtures, MIN_BITS),
             fixtures_middle_subsequences=(scenario_fixtures, MIDDLE_BITS))
    s.update({c[0]: (scenario_large, c) for c in LARGE})
    s.update(two_decoders=(scenario_two_decoders,), unsupported_in_a_batch=(scenario_unsupported_in_a_batch,),
             bytes_behind_the_last_block=(scenario_bytes_behind_the_last_block,), orientations=(scenario_orientations,), load_jpegs=(scenario_load_jpegs,), refusals=(scenario_refusals,))
    return s


if __name__ == "__main__":
    ctx = capi.Context(0)
    res, device_error = {}, False
    for name, (fn, *args) in scenarios().items():
        try:
            fn(ctx, *args)
            res[name] = "ok"
        except AssertionError:
            res[name] = traceback.format_exc()
        except Exception:  # a device error: nothing more runs on that device
            res[name] = traceback.format_exc()
            device_error = True
            break
    for name in scenarios():
        res.setdefault(name, "not run: an earlier scenario ended in an error")
    print(json.dumps(res), flush=True)
    if not device_error:
        ctx.close()
