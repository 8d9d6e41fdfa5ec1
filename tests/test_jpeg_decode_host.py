"""Baseline JPEG decoding in host loops (csrc/jpeg_decode.hpp run by host/jpeg_decode.cpp) against
libjpeg-turbo's pixels, byte for byte: the committed files under tests/golden/jpeg_decode/ with the pixels Pillow decoded
from them (scripts/make_jpeg_decode_golden.py), live Pillow where it is importable - the shapes of jpeg_fixtures up to
64 x 80 in four samplings and four contents, the qualities, optimised tables and restart intervals, the orientations - the
unsupported classes, damaged files, and the same through a stand-alone program under the address and undefined-behaviour
sanitizers (tests/jpeg_decode_driver.cpp)."""
import warnings

import numpy as np
import pytest

import jpeg_decode_fixtures as D
import jpeg_fixtures as F
from opencalibration_amd import capi, host

pillow = pytest.mark.skipif(not D.have_pillow(), reason="Pillow is not importable")
GOLDEN = sorted(D.golden_files())


@pytest.mark.parametrize("name", GOLDEN)
def test_equals_the_committed_pixels(name):
    data = D.golden_bytes(name)
    D.check_golden(name, host.decode_jpeg(data), oriented=True)
    D.check_golden(name, host.decode_jpeg(data, apply_orientation=False), oriented=False)


def test_info_of_the_committed_files():
    i = host.jpeg_info(D.golden_bytes("sample_right"))
    assert i == dict(width=480, height=640, components=1, sampling=(1, 1), restart_interval=0, orientation=8, status="ok")
    i = host.jpeg_info(D.golden_bytes("sample_right"), apply_orientation=False)
    assert (i["width"], i["height"], i["orientation"]) == (640, 480, 8)
    assert host.jpeg_info(D.golden_bytes("sample_down-mirrored"))["orientation"] == 4
    i = host.jpeg_info(D.golden_bytes("sample_bb-android"))
    assert (i["width"], i["height"], i["components"], i["sampling"]) == (10, 6, 3, (2, 2))
    assert host.jpeg_info(D.golden_bytes("noise_33x47_422"))["sampling"] == (2, 1)
    assert host.jpeg_info(D.golden_bytes("noise_33x47_444"))["sampling"] == (1, 1)
    assert host.jpeg_info(D.golden_bytes("noise_33x47_422_restart_1_block"))["restart_interval"] == 1
    assert host.jpeg_info(D.golden_bytes("noise_33x47_420_restart_2_blocks"))["restart_interval"] == 2
    assert host.jpeg_info(D.golden_bytes("noise_33x47_420_restart_3_blocks"))["restart_interval"] == 3
    assert host.jpeg_info(D.golden_bytes("noise_48x64_420_restart_1_row"))["restart_interval"] == 4
    for name, o, _ in D.EXIF_GOLDEN:
        assert host.jpeg_info(D.golden_bytes(name))["orientation"] == o


def test_the_fixtures_hold_what_they_are_for():
    scan = D.golden_bytes(D.FF00_FIXTURE)
    assert b"\xff\x00" in scan[D.segments(scan)[-1][1]:]                       # stuffed bytes in the scan
    exif = D.golden_bytes(D.EXIF_THUMBNAIL_FIXTURE)
    marker, at, length = next(seg for seg in D.segments(exif) if seg[0] == 0xE1)
    assert b"\xff\xd8" in exif[at + 4:at + 2 + length]        # a second SOI inside APP1 ...
    assert b"\xff\xc0" in exif[at + 4:at + 2 + length]                           # ... and a frame header ahead of the real one
    optimised = D.golden_bytes("noise_48x64_420_optimized")
    assert max(ln for m, at, ln in D.segments(optimised) if m == 0xC4) < 200     # not the Annex K tables
    assert b"\xff\xd0" in D.golden_bytes("noise_33x47_420_restart_2_blocks")  # intervals of 2 MCUs in MCU rows of 3


@pillow
@pytest.mark.parametrize("sampling", D.SAMPLINGS)
def test_equals_live_pillow_on_every_shape(sampling):
    for h, w in D.SHAPES:
        for kind in F.CONTENTS:
            data = D.pillow_encode(F.content(kind, h, w, h * 131 + w), sampling)
            assert np.array_equal(host.decode_jpeg(data), D.pillow_decode(data)), (h, w, kind)


@pillow
@pytest.mark.parametrize("sampling", D.SAMPLINGS)
def test_equals_live_pillow_across_qualities_tables_and_restarts(sampling):
    for h, w in [(1, 1), (17, 33), (33, 47), (48, 64)]:
        rgb = F.noise(h, w, 7 * h + w)
        for quality in (1, 50, 95, 100):
            for options in ({}, {"optimize": True}, {"restart_marker_blocks": 1}, {"restart_marker_blocks": 3}, {"restart_marker_blocks": 5},
                            {"restart_marker_rows": 1}):
                data = D.pillow_encode(rgb, sampling, quality, **options)
                assert np.array_equal(host.decode_jpeg(data), D.pillow_decode(data)), (h, w, quality, options)


@pillow
def test_orientations_on_a_non_square_image():
    for o in range(1, 9):
        for big_endian in (False, True):
            data = D.exif_file(o, big_endian, with_thumbnail=o == 6)
            info = host.jpeg_info(data)
            assert info["orientation"] == o and (info["height"], info["width"]) == (D.ORIENTED_SHAPE if o < 5 else D.ORIENTED_SHAPE[::-1])
            assert np.array_equal(host.decode_jpeg(data), D.pillow_decode(data)), o
            plain = host.decode_jpeg(data, apply_orientation=False)
            assert plain.shape[:2] == D.ORIENTED_SHAPE and np.array_equal(plain, D.pillow_decode(data, apply_orientation=False)), o


@pillow
def test_round_trip_through_the_encoder():
    for kind in F.CONTENTS:
        data = host.encode_jpeg(F.content(kind, 33, 47, 4))
        assert np.array_equal(host.decode_jpeg(data), D.pillow_decode(data)), kind


def _unsupported():
    cases = D.unsupported_by_patch(D.golden_bytes("noise_33x47_444"), D.golden_bytes("noise_33x47_420"))
    if D.have_pillow():
        from PIL import Image
        import io

        rgb = F.noise(33, 47, 1)
        cases["progressive"] = D.pillow_encode(rgb, "420", progressive=True)
        f = io.BytesIO()
        Image.fromarray(F.rgba_of(rgb), "CMYK").save(f, format="JPEG")
        cases["four_components"] = f.getvalue()
    return cases


def test_unsupported_files_say_so():
    cases = _unsupported()
    assert len(cases) >= 8
    with host.JpegDecoder() as d:
        batch = d.decode(list(cases.values()))
    for name, status, data in zip(cases, batch.status, cases.values()):
        assert status == "unsupported" and host.jpeg_info(data)["status"] == "unsupported", name
        with pytest.raises(capi.OchipError, match="unsupported"):
            host.decode_jpeg(data)


def test_a_batch_keeps_the_neighbours_of_a_refused_file():
    good, bad = D.golden_bytes("noise_33x47_420"), _unsupported()["arithmetic"]
    with host.JpegDecoder() as d:
        b = d.decode([good, bad, D.golden_bytes("noise_33x47_gray"), good[:300], good])
    assert b.status == ["ok", "unsupported", "ok", "corrupt", "ok"] and b.shapes[1] is None and b.offsets[3] is None
    D.check_golden("noise_33x47_420", b.image(0))
    D.check_golden("noise_33x47_gray", b.image(2))
    D.check_golden("noise_33x47_420", b.image(4))
    assert b.pixels.size == 3 * 33 * 47 * 3


def test_a_short_scan_is_corrupt():
    for name in D.DAMAGED:
        data = D.golden_bytes(name)
        assert host.jpeg_info(data[:len(data) // 2])["status"] in ("ok", "corrupt")
        with pytest.raises(capi.OchipError, match="corrupt"):
            host.decode_jpeg(data[:len(data) * 3 // 4])
        D.check_golden(name, host.decode_jpeg(data[:-2]))   # the EOI alone is missing: the scan is whole, so is the picture


def _refused_by_header():
    """name -> bytes: files whose headers alone are not a JPEG's - Huffman counts that are no prefix code, a frame header
    that promises more blocks than the scan has bits for"""
    cases = D.bad_huffman_tables(D.golden_bytes("noise_33x47_420"))
    cases["65535_x_65535"] = D.huge_header(D.golden_bytes("noise_33x47_420"))
    cases["65535_x_65535_gray"] = D.huge_header(D.golden_bytes("noise_33x47_gray"))
    return cases


def test_headers_that_are_no_jpegs_are_corrupt():
    cases = _refused_by_header()
    with host.JpegDecoder() as d:
        b = d.decode(list(cases.values()))
    for name, status, data in zip(cases, b.status, cases.values()):
        assert status == "corrupt" and host.jpeg_info(data)["status"] == "corrupt", name
    assert b.offsets == [None] * len(cases) and b.pixels.size == 1


def test_bytes_behind_the_last_block_are_not_read():
    for name in ("noise_33x47_420", "noise_33x47_gray", "noise_48x64_420_restart_1_row"):
        D.check_golden(name, host.decode_jpeg(D.bytes_behind_the_last_block(D.golden_bytes(name))))


def test_a_corrupt_scan_keeps_its_room():
    good = D.golden_bytes("noise_33x47_420")
    with host.JpegDecoder() as d:
        b = d.decode([good[:len(good) * 3 // 4], good], out=np.zeros(2 * 33 * 47 * 3, np.uint8))
    assert b.status == ["corrupt", "ok"] and b.offsets == [None, 33 * 47 * 3]
    D.check_golden("noise_33x47_420", b.image(1))


def test_damaged_files_give_a_status_or_a_picture():
    for k, name in enumerate(D.DAMAGED):
        files = D.damaged(D.golden_bytes(name), seed=k)
        with host.JpegDecoder() as d:
            b = d.decode(files)
        assert len(b.status) == len(files) and set(b.status) <= {"ok", "unsupported", "corrupt"}
        for i, s in enumerate(b.status):
            assert (b.image(i).ndim == 3) if s == "ok" else (b.shapes[i] is None)
        assert "corrupt" in b.status


def test_misuse_is_refused():
    with pytest.raises(capi.OchipError, match="subsequence_bits 33"):
        host.JpegDecoder(subsequence_bits=33)
    good = D.golden_bytes("noise_33x47_420")
    with host.JpegDecoder() as d:
        with pytest.raises(capi.OchipError, match="the output holds 100"):
            d.decode([good], out=np.zeros(100, np.uint8))
        assert d.decode([]).status == []
        assert d.L.och_jpeg_decoder_decode(d.h, 65536, None, None, 1, None, 0, None, None, None) == -1
        assert "65536 files, at most 65535" in d._error()
        dead = d.h
    L = host.load()
    assert L.och_jpeg_decoder_decode(dead, 0, None, None, 1, None, 0, None, None, None) == -1
    assert "not a live" in L.och_jpeg_decode_last_error().decode()
    L.och_jpeg_decoder_destroy(dead)                         # a dead handle is refused, not followed


def test_the_stand_alone_program_under_the_sanitizers():
    """every committed file, then the truncations and mutations: the program ends clean and agrees with the library"""
    if not D.driver()[1]:
        warnings.warn("the sanitizer runtime does not link here: the stand-alone program ran without -fsanitize, memory safety unchecked")
    names = GOLDEN
    files = [D.golden_bytes(n) for n in names]
    for (status, pixels), name in zip(D.run_driver(files), names):
        assert status == "ok", name
        D.check_golden(name, pixels)
    for (status, pixels), name in zip(D.run_driver(files, apply_orientation=False), names):
        D.check_golden(name, pixels, oriented=False)
    files = [f for k, name in enumerate(D.DAMAGED) for f in D.damaged(D.golden_bytes(name), seed=k)] + list(_unsupported().values()) + \
        list(_refused_by_header().values()) + [D.bytes_behind_the_last_block(D.golden_bytes("noise_33x47_420"))]
    with host.JpegDecoder() as d:
        b = d.decode(files)
    got = D.run_driver(files)
    assert [s for s, _ in got] == b.status
    for i, (s, pixels) in enumerate(got):
        if s == "ok":
            assert np.array_equal(pixels, b.image(i))
