"""Shared by test_jpeg_decode_host.py, test_gpu_jpeg_decode.py, jpeg_decode_gpu_child.py and
scripts/make_jpeg_decode_golden.py: the committed files with their expected pixels, the header patches that make the
unsupported classes, the damaged files, and the stand-alone driver.  Nothing here decodes with the library; Pillow is
imported only by the functions that need it."""
import functools
import hashlib
import io
import json
import os
import struct
import subprocess
import tempfile

import numpy as np

import jpeg_fixtures as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden", "jpeg_decode")
TEXTURE_DIR = F.GOLDEN_DIR
MANIFEST = os.path.join(GOLDEN_DIR, "expected.json")
MAX_FIXTURE_BYTES = 64 * 1024
SAMPLINGS = ["444", "422", "420", "gray"]
SHAPES = [s for s in F.SHAPES if s[0] <= 64 and s[1] <= 80]
ORIENTED_SHAPE = (24, 40)
# (name, content, height, width, seed, sampling, quality, save options) of the files Pillow writes for the golden set
PILLOW_GOLDEN = [
    ("noise_33x47_444", "noise", 33, 47, 5, "444", 95, {}),
    ("noise_33x47_422", "noise", 33, 47, 5, "422", 95, {}),
    ("noise_33x47_420", "noise", 33, 47, 5, "420", 95, {}),
    ("noise_33x47_gray", "noise", 33, 47, 5, "gray", 95, {}),
    ("ramp_31x33_420_q50", "ramp", 31, 33, 0, "420", 50, {}),
    ("noise_17x33_420_q1", "noise", 17, 33, 2, "420", 1, {}),
    ("noise_48x64_420_q100", "noise", 48, 64, 2, "420", 100, {}),
    ("flat_48x64_420_q1", "flat", 48, 64, 0, "420", 1, {}),
    ("checker_32x48_422_q50", "checker", 32, 48, 0, "422", 50, {}),
    ("noise_48x64_420_optimized", "noise", 48, 64, 3, "420", 95, {"optimize": True}),
    ("noise_33x47_422_restart_1_block", "noise", 33, 47, 6, "422", 95, {"restart_marker_blocks": 1}),
    ("noise_33x47_420_restart_2_blocks", "noise", 33, 47, 7, "420", 95, {"restart_marker_blocks": 2}),
    ("noise_33x47_420_restart_3_blocks", "noise", 33, 47, 10, "420", 95, {"restart_marker_blocks": 3}),
    ("noise_48x64_420_restart_1_row", "noise", 48, 64, 8, "420", 95, {"restart_marker_rows": 1}),
    ("noise_2x2_420", "noise", 2, 2, 9, "420", 95, {}),
    ("noise_1x1_gray", "noise", 1, 1, 9, "gray", 95, {}),
]
# the EXIF files: orientation, byte order; the first carries a thumbnail JPEG inside APP1
EXIF_GOLDEN = [(f"ramp_24x40_420_orientation_{o}", o, o % 2 == 0) for o in range(1, 9)]
REFERENCE_SAMPLES = ["right.jpg", "down-mirrored.jpg", "bb-android.jpg", "test2.jpg"]
FF00_FIXTURE = "noise_48x64_420_q100"
EXIF_THUMBNAIL_FIXTURE = "ramp_24x40_420_orientation_1"
DAMAGED = ["noise_33x47_420", "noise_33x47_422_restart_1_block", "noise_48x64_420_optimized"]


def have_pillow():
    try:
        import PIL  # noqa: F401
        return True
    except ImportError:
        return False


def pillow_encode(rgb, sampling="420", quality=95, **options):
    from PIL import Image

    f = io.BytesIO()
    if sampling == "gray":
        Image.fromarray(rgb).convert("L").save(f, format="JPEG", quality=quality, **options)
    else:
        Image.fromarray(rgb).save(f, format="JPEG", quality=quality, subsampling={"444": 0, "422": 1, "420": 2}[sampling], **options)
    return f.getvalue()


def pillow_decode(data, apply_orientation=True):
    """what cv::imread gives, through Pillow: libjpeg-turbo's default decode, the EXIF orientation applied, B G R"""
    from PIL import Image, ImageOps

    im = Image.open(io.BytesIO(data))
    if apply_orientation:
        im = ImageOps.exif_transpose(im)
    return np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])


def exif_segment(orientation, thumbnail=None, big_endian=False):
    """"Exif\\0\\0" and a TIFF with the orientation in IFD0 and, with a thumbnail, an IFD1 that points at it"""
    e = ">" if big_endian else "<"
    ifd0 = struct.pack(e + "H", 1) + struct.pack(e + "HHIHH", 0x0112, 3, 1, orientation, 0)
    ifd1_at = 8 + len(ifd0) + 4
    if thumbnail is None:
        body = ifd0 + struct.pack(e + "I", 0)
    else:
        thumb_at = ifd1_at + 2 + 2 * 12 + 4
        ifd1 = struct.pack(e + "H", 2) + struct.pack(e + "HHII", 0x0201, 4, 1, thumb_at) + struct.pack(e + "HHII", 0x0202, 4, 1, len(thumbnail)) + \
            struct.pack(e + "I", 0)
        body = ifd0 + struct.pack(e + "I", ifd1_at) + ifd1 + thumbnail
    return b"Exif\0\0" + (b"MM\0*" if big_endian else b"II*\0") + struct.pack(e + "I", 8) + body


def exif_file(orientation, big_endian, with_thumbnail):
    h, w = ORIENTED_SHAPE
    thumb = pillow_encode(F.ramp(6, 10), "420", 50) if with_thumbnail else None
    return pillow_encode(F.ramp(h, w), "420", 95, exif=exif_segment(orientation, thumb, big_endian))


def segments(data):
    """(marker, offset of the FF, length of the segment with its two length bytes) up to and with SOS"""
    out, at = [], 2
    while True:
        assert data[at] == 0xFF
        marker, length = data[at + 1], int.from_bytes(data[at + 2:at + 4], "big")
        out.append((marker, at, length))
        if marker == 0xDA:
            return out
        at += 2 + length


def _segment(data, marker):
    return next(s for s in segments(data) if s[0] == marker)


def patched(data, at, new):
    return data[:at] + bytes(new) + data[at + len(bytes(new)):]


def unsupported_by_patch(base444, base420):
    """name -> bytes: the unsupported classes made from a 4:4:4 and a 4:2:0 baseline file by changing header bytes"""
    _, sof, _ = _segment(base420, 0xC0)
    _, sos, sos_len = _segment(base444, 0xDA)
    _, sof4, _ = _segment(base444, 0xC0)
    out = {
        "arithmetic": patched(base420, sof + 1, [0xC9]),
        "twelve_bits": patched(base420, sof + 4, [12]),
        "sampling_440": patched(base420, sof + 11, [0x12]),
        "sampling_411": patched(base420, sof + 11, [0x41]),
        "several_scans": base444[:sos] + bytes([0xFF, 0xDA, 0x00, 0x08, 0x01, 0x01, 0x00, 0x00, 0x3F, 0x00]) + base444[sos + 2 + sos_len:],
        "adobe_transform_0": base444[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + base444[2:],
    }
    rgb = patched(base444, sof4 + 10, [ord("R")])
    rgb = patched(rgb, sof4 + 13, [ord("G")])
    rgb = patched(rgb, sof4 + 16, [ord("B")])
    rgb = patched(rgb, sos + 5, [ord("R")])
    rgb = patched(rgb, sos + 7, [ord("G")])
    out["component_ids_rgb"] = patched(rgb, sos + 9, [ord("B")])
    wide, at = base420[:2], 2
    for marker, off, length in segments(base420):
        wide += base420[at:off]
        seg = base420[off:off + 2 + length]
        if marker == 0xDB:
            body, new, k = seg[4:], b"", 0
            while k < len(body):
                new += bytes([0x10 | body[k]]) + b"".join(bytes([0, v]) for v in body[k + 1:k + 65])
                k += 65
            seg = b"\xff\xdb" + (len(new) + 2).to_bytes(2, "big") + new
        wide += seg
        at = off + 2 + length
    out["dqt_16_bits"] = wide + base420[at:]
    return out


def damaged(data, seed, count=12):
    """truncations and byte mutations of a file: a list of bytes objects, the same for a seed"""
    rng = np.random.default_rng(seed)
    out = [data[:n] for n in (0, 1, 2, 3, len(data) // 4, len(data) // 2, len(data) * 3 // 4, len(data) - 2, len(data) - 1)]
    for _ in range(count):
        b = bytearray(data)
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(2, len(b)))] = int(rng.integers(0, 256))
        out.append(bytes(b))
    return out


def bad_huffman_tables(base):
    """name -> bytes: the file with a DHT segment ahead of its own whose counts are no prefix code - more codes of length 1,
    and of length 2, than there are - on table id 3"""
    def dht(counts, values):
        body = bytes([0x03]) + bytes(counts + [0] * (16 - len(counts))) + bytes(values)
        return b"\xff\xc4" + (len(body) + 2).to_bytes(2, "big") + body

    return {"three_codes_of_length_1": base[:2] + dht([3], [1, 2, 3]) + base[2:],
            "255_codes_of_length_1": base[:2] + dht([255], list(range(255))) + base[2:],
            "two_of_length_1_one_of_length_2": base[:2] + dht([2, 1], [1, 2, 3]) + base[2:],
            "five_codes_of_length_2": base[:2] + dht([0, 5], [1, 2, 3, 4, 5]) + base[2:],
            "only_the_table": base[:2] + dht([3], [1, 2, 3]) + b"\xff\xd9"}


def huge_header(base):
    """the file with 65 535 x 65 535 in its frame header: far more blocks than the scan has bits for"""
    _, sof, _ = _segment(base, 0xC0)
    return patched(base, sof + 5, [0xFF, 0xFF, 0xFF, 0xFF])


def bytes_behind_the_last_block(base, count=40):
    """the file with `count` zero bytes between its scan and EOI: decodable symbols that belong to no block"""
    assert base.endswith(b"\xff\xd9")
    return base[:-2] + bytes(count) + b"\xff\xd9"


def golden_files():
    """name -> path of every committed input: Pillow's, the EXIF ones, the reference's samples, this project's encoder's"""
    out = {name: os.path.join(GOLDEN_DIR, name + ".jpg") for name, *_ in PILLOW_GOLDEN}
    out.update({name: os.path.join(GOLDEN_DIR, name + ".jpg") for name, _, _ in EXIF_GOLDEN})
    out.update({"sample_" + s[:-4]: os.path.join(GOLDEN_DIR, "sample_" + s) for s in REFERENCE_SAMPLES})
    out.update({"texture_" + F.golden_name(c)[:-4]: os.path.join(TEXTURE_DIR, F.golden_name(c)) for c in F.GOLDEN})
    return out


@functools.lru_cache(maxsize=None)
def golden_bytes(name):
    with open(golden_files()[name], "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def manifest():
    with open(MANIFEST) as f:
        return json.load(f)


def sha256(pixels):
    return hashlib.sha256(np.ascontiguousarray(pixels).tobytes()).hexdigest()


def check_golden(name, pixels, oriented=True):
    """asserts that pixels are the committed expectation of a golden file (oriented: with the EXIF orientation applied)"""
    want = manifest()[name]["oriented" if oriented else "plain"]
    assert list(pixels.shape) == want["shape"], (name, pixels.shape, want["shape"])
    if "file" in want:
        stored = np.fromfile(os.path.join(GOLDEN_DIR, want["file"]), np.uint8).reshape(want["shape"])
        assert np.array_equal(pixels, stored), (name, int((pixels != stored).sum()))
    else:
        assert sha256(pixels) == want["sha256"], name


@functools.lru_cache(maxsize=None)
def driver():
    """The stand-alone program over the host route (tests/jpeg_decode_driver.cpp), built once per process with the address
    and undefined-behaviour sanitizers; without them where their runtime does not link.  Returns (path, sanitized)."""
    exe = os.path.join(tempfile.mkdtemp(prefix="jpeg_decode_driver_"), "jpeg_decode_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-DOCHIP_JPEG_DECODE_STANDALONE", "-I", os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "jpeg_decode_driver.cpp"), os.path.join(ROOT, "opencalibration_amd", "csrc", "host", "jpeg_decode.cpp")]
    if subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode == 0:
        return exe, True
    subprocess.run(cmd, check=True)
    return exe, False


def run_driver(files, apply_orientation=True):
    """The driver over a list of bytes objects: a list of (status name, pixels or None)."""
    exe, _ = driver()
    d = tempfile.mkdtemp(prefix="jpeg_decode_run_")
    lines = []
    for i, data in enumerate(files):
        with open(os.path.join(d, f"{i}.jpg"), "wb") as f:
            f.write(data)
        lines.append(f"{os.path.join(d, f'{i}.jpg')} {os.path.join(d, f'{i}.bgr')} {int(apply_orientation)}")
    with open(os.path.join(d, "list.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, os.path.join(d, "list.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = []
    rows = r.stdout.strip().splitlines()
    assert len(rows) == len(files)
    for i, row in enumerate(rows):
        status, w, h = row.split()
        out.append((status, np.fromfile(os.path.join(d, f"{i}.bgr"), np.uint8).reshape(int(h), int(w), 3) if status == "ok" else None))
    return out
