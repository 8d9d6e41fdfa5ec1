"""host.jpeg_metadata against Pillow's reading of the same files: the committed expectations, live
Pillow on the committed files, the reference's EXIF samples and files written here, and - cut at every byte of the APP1
segments or with their IFD offsets and counts overwritten - never anything but "ok", "absent" or "corrupt".  The mapping
from Pillow's tags to image_metadata is scripts/make_survey_golden.py's pillow_metadata, the one that wrote the committed
expectations."""
import functools
import glob
import importlib.util
import json
import math
import os
import random
import struct
import subprocess
import tempfile
import warnings

import pytest

from opencalibration_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURVEY_DIR = os.path.join(ROOT, "tests", "golden", "survey_files")
SAMPLES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "jpeg_decode", "sample_*.jpg")))


@functools.lru_cache(maxsize=None)
def golden_script():
    spec = importlib.util.spec_from_file_location("make_survey_golden", os.path.join(ROOT, "scripts", "make_survey_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def expected():
    with open(os.path.join(SURVEY_DIR, "expected.json")) as f:
        return json.load(f)


NAMES = ["le_north_east_35mm", "be_south_west_cm", "le_inch", "dji_attributes", "dji_elements", "camera_packet", "xmp_before_exif",
         "thumbnail_in_app1", "no_app1", "zero_denominator"]


def committed(name):
    with open(os.path.join(SURVEY_DIR, name + ".jpg"), "rb") as f:
        return f.read()


def same(a, b):
    """== with NaN equal to NaN, key order included"""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return a == b and type(a) is type(b)


KEYS = dict(camera_info=["dimensions", "focal_length_px", "principal", "make", "model", "serial_no", "lens_make", "lens_model"],
            capture_info=["latitude", "longitude", "altitude", "relative_altitude", "roll", "pitch", "yaw", "accuracy_xy",
                          "accuracy_z", "datum", "timestamp", "datestamp"])


def test_the_committed_list_is_the_directory():
    assert sorted(NAMES) == sorted(expected()) == sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(SURVEY_DIR, "*.jpg")))


@pytest.mark.parametrize("name", NAMES)
def test_equals_the_committed_expectation(name):
    md, status = host.jpeg_metadata(committed(name), want_status=True)
    assert list(md) == list(KEYS) and all(list(md[k]) == KEYS[k] for k in KEYS)   # write_default_metadata's layout and order
    assert status == expected()[name]["status"]
    assert same(md, expected()[name]["metadata"]), (md, expected()[name]["metadata"])
    assert same(host.jpeg_metadata(os.path.join(SURVEY_DIR, name + ".jpg")), md)  # a path reads the same


def test_what_the_cases_are_there_for():
    """each fixture shows the rule it was written for"""
    md = {n: host.jpeg_metadata(committed(n)) for n in NAMES}
    cam, cap = {n: md[n]["camera_info"] for n in NAMES}, {n: md[n]["capture_info"] for n in NAMES}
    assert cap["le_north_east_35mm"]["latitude"] > 0 and cap["le_north_east_35mm"]["longitude"] > 0
    assert cap["be_south_west_cm"]["latitude"] < 0 and cap["be_south_west_cm"]["longitude"] < 0
    assert cap["le_north_east_35mm"]["altitude"] == 432.1 and cap["be_south_west_cm"]["altitude"] == -12.5    # AltRef 0 and 1
    assert cap["le_north_east_35mm"]["timestamp"] == "2024:05:01 10:00:0137"                                  # original + subsec
    assert cap["be_south_west_cm"]["timestamp"] == "2024:05:01 11 0 12.34" and cap["be_south_west_cm"]["datum"] == "WGS-84"
    assert cam["le_north_east_35mm"]["focal_length_px"] == 24 / 43.27 * math.hypot(64, 48)
    assert cam["be_south_west_cm"]["focal_length_px"] == 8.8 / (10 / (12500 / 3))                              # unit 3: centimetres
    assert cam["le_inch"]["focal_length_px"] == 5.0 / (25.4 / 10583.0)
    for n in ("dji_attributes", "dji_elements", "xmp_before_exif"):
        assert cam[n]["focal_length_px"] == 3666.666504 and cam[n]["principal"] == [1824.0, 2736.0], n          # Y, X: swapped
        assert cap[n]["altitude"] == 80.10 and cap[n]["accuracy_z"] == 0.0, n               # the relative altitude replaces it
        assert (cap[n]["roll"], cap[n]["pitch"], cap[n]["yaw"]) == (0.0, -89.9, -112.4), n
    assert cam["xmp_before_exif"]["dimensions"] == [64, 48]                                  # tiff:ImageWidth / ImageLength
    assert cap["camera_packet"]["pitch"] == 3.25 - 90 and cap["camera_packet"]["accuracy_xy"] == 0.02
    assert cap["camera_packet"]["accuracy_z"] == 3 / 100
    assert cam["thumbnail_in_app1"]["make"] == "DJI" and cap["thumbnail_in_app1"]["altitude"] == 80.10      # not the thumbnail's
    assert math.isnan(cap["zero_denominator"]["altitude"]) and cap["zero_denominator"]["latitude"] == 10.0
    assert cam["zero_denominator"]["focal_length_px"] == 24 / 43.27 * 80


def live(data):
    md, status = golden_script().pillow_metadata(data)
    got, got_status = host.jpeg_metadata(data, want_status=True)
    assert got_status == status
    assert same(got, md), (got, md)
    return got


@pytest.mark.parametrize("name", NAMES)
def test_equals_live_pillow_on_the_committed_files(name):
    live(committed(name))


@pytest.mark.parametrize("path", SAMPLES, ids=[os.path.basename(p) for p in SAMPLES])
def test_equals_live_pillow_on_the_reference_samples(path):
    with open(path, "rb") as f:
        live(f.read())


def test_the_reference_samples_are_four():
    assert len(SAMPLES) == 4


def test_equals_live_pillow_on_files_written_here():
    S = golden_script()
    rng = random.Random(20240501)
    for k in range(12):
        lat, lon = rng.uniform(-80, 80), rng.uniform(-179, 179)
        gps = S.gps_ifd(lat, lon, S.R(rng.randrange(1, 900000), 1000), rng.randrange(2),
                        date="2024:06:%02d" % (k + 1) if k % 2 else None, time=(S.R(k, 1), S.R(59, 1), S.R(5999, 100)))
        exif = {0xa002: S.W, 0xa003: S.H}
        if k % 3 == 0:
            exif[0xa405] = rng.randrange(10, 200)
        elif k % 3 == 1:
            exif.update({0x920a: S.R(rng.randrange(20, 500), 10), 0xa20e: S.R(rng.randrange(1000, 90000), 7), 0xa210: 2 + k % 2})
        segs = [S.exif_bytes({0x010f: "DJI" if k % 4 == 0 else "Maker %d" % k, 0x0110: "M%d" % k}, exif, gps, big_endian=bool(k & 1))]
        if k % 4 in (0, 3):
            dji = dict(S.DJI)
            dji["drone-dji:RelativeAltitude"] = "%+.2f" % rng.uniform(-5, 120)
            segs.append(S.xmp_packet(dji, elements=bool(k & 2), about="DJI Meta Data" if k % 4 == 3 else ""))
        md = live(S.splice(S.base_jpeg(seed=20 + k), segs))
        assert abs(md["capture_info"]["latitude"] - lat) < 1e-7 and abs(md["capture_info"]["longitude"] - lon) < 1e-7


# ---- damaged files ----------------------------------------------------------------------------------------------------
def app1_span(data):
    """[first byte of the first APP1 marker, one past the last APP1 segment)"""
    at, first, last = 2, None, None
    while at + 4 <= len(data) and data[at] == 0xFF and data[at + 1] not in (0xDA, 0xD9):
        n = struct.unpack(">H", data[at + 2:at + 4])[0]
        if data[at + 1] == 0xE1:
            first, last = at if first is None else first, at + 2 + n
        at += 2 + n
    return first, last


def truncations(data):
    first, last = app1_span(data)
    return [] if first is None else [data[:cut] for cut in range(first, last + 1)]


def ifd_fields(data):
    """(offset in the file, width) of the TIFF header's IFD0 offset and of every count, entry count, value / offset field of
    IFD0, the Exif IFD and the GPS IFD of the file's first Exif segment, with the byte order"""
    t = data.find(b"Exif\0\0") + 6
    order = "<" if data[t:t + 2] == b"II" else ">"
    fields, todo, seen = [(t + 4, 4)], [struct.unpack(order + "I", data[t + 4:t + 8])[0]], set()
    while todo:
        ifd = todo.pop()
        if ifd in seen or t + ifd + 2 > len(data):
            continue
        seen.add(ifd)
        fields.append((t + ifd, 2))
        for i in range(struct.unpack(order + "H", data[t + ifd:t + ifd + 2])[0]):
            e = t + ifd + 2 + 12 * i
            if e + 12 > len(data):
                break
            fields += [(e + 2, 2), (e + 4, 4), (e + 8, 4)]
            if struct.unpack(order + "H", data[e:e + 2])[0] in (0x8769, 0x8825):
                todo.append(struct.unpack(order + "I", data[e + 8:e + 12])[0])
    return fields, order


def mutations(data, rng, count=150):
    fields, order = ifd_fields(data)
    out = []
    for _ in range(count):
        b = bytearray(data)
        for at, width in rng.sample(fields, rng.choice((1, 1, 2, 3))):
            v = rng.choice((0, 1, 2, 7, 8, 0xFFFF, 0x7FFFFFFF, 0xFFFFFFFF, 0xFFFFFFF8, rng.randrange(1 << 32), rng.randrange(4096)))
            b[at:at + width] = struct.pack(order + ("H" if width == 2 else "I"), v & (0xFFFF if width == 2 else 0xFFFFFFFF))
        out.append(bytes(b))
    return out


@functools.lru_cache(maxsize=None)
def damaged():
    rng = random.Random(4023)
    out = []
    for name in NAMES:
        data = committed(name)
        out += truncations(data)
        if b"Exif\0\0" in data:
            out += mutations(data, rng)
    return out


def test_truncated_at_every_byte_of_the_app1_segments():
    total = 0
    for name in NAMES:
        cuts = truncations(committed(name))
        assert cuts or name == "no_app1"
        for cut in cuts:
            md, status = host.jpeg_metadata(cut, want_status=True)
            assert status in ("ok", "absent", "corrupt")
            if status != "ok":
                assert same(md, expected()["no_app1"]["metadata"])  # the defaults
        total += len(cuts)
    assert total > 3000


def test_seeded_mutations_of_the_ifd_offsets_and_counts():
    rng = random.Random(77)
    seen = set()
    for name in NAMES:
        data = committed(name)
        if b"Exif\0\0" not in data:
            continue
        for bad in mutations(data, rng):
            md, status = host.jpeg_metadata(bad, want_status=True)
            assert status in ("ok", "absent", "corrupt")
            seen.add(status)
    assert {"ok", "corrupt"} <= seen


def test_not_a_jpeg_and_nothing_at_all():
    for data in (b"", b"\xff", b"\xff\xd8", b"II*\0" + bytes(64), bytes(100)):
        md, status = host.jpeg_metadata(data, want_status=True)
        assert status == "corrupt" and same(md, expected()["no_app1"]["metadata"])


@functools.lru_cache(maxsize=None)
def driver():
    """tests/image_metadata_driver.cpp with the address and undefined-behaviour sanitizers; without them where their runtime
    does not link.  Returns (path, sanitized)."""
    exe = os.path.join(tempfile.mkdtemp(prefix="image_metadata_driver_"), "image_metadata_driver")
    src = os.path.join(ROOT, "opencalibration_amd", "csrc", "host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "image_metadata_driver.cpp"),
           os.path.join(src, "image_metadata.cpp"), os.path.join(src, "geo_coord.cpp")]
    if subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode == 0:
        return exe, True
    subprocess.run(cmd, check=True)
    return exe, False


def test_the_stand_alone_program_under_the_sanitizers():
    """every committed, truncated and mutated file, each in a heap block of exactly its size: the run is clean and the
    statuses and fields are the library's"""
    exe, sanitized = driver()
    if not sanitized:
        warnings.warn("the sanitizer runtime does not link here: the stand-alone program ran without -fsanitize, memory safety unchecked")
    files = [committed(n) for n in NAMES] + damaged() + [b"", b"\xff\xd8"]
    pack = os.path.join(tempfile.mkdtemp(prefix="image_metadata_pack_"), "pack.bin")
    with open(pack, "wb") as f:
        for data in files:
            f.write(struct.pack("<I", len(data)) + data)
    r = subprocess.run([exe, pack], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-4000:]
    rows = r.stdout.strip().splitlines()
    assert len(rows) == len(files)
    for row, data in zip(rows, files):
        status, w, h, focal, lat, n_make, n_time, round_trip = row.split()
        md, st = host.jpeg_metadata(data, want_status=True)
        assert host.METADATA_STATUS[int(status)] == st
        assert [int(w), int(h)] == md["camera_info"]["dimensions"]
        assert same(float(focal), md["camera_info"]["focal_length_px"]) and same(float(lat), md["capture_info"]["latitude"])
        # the binding stops a string at a NUL and turns a byte that is no UTF-8 into one character: never more characters
        assert int(n_make) >= len(md["camera_info"]["make"]) and int(round_trip) == 1
