"""The textured OBJ's JPEG texture in host loops (csrc/jpeg_encode.hpp run by host/jpeg_encode.cpp)
against libjpeg-turbo's bytes: the files Pillow wrote, committed under tests/golden/jpeg_texture/ (scripts/make_jpeg_golden.py),
always, and live Pillow where it is installed.  Byte for byte; no device."""
import io
import os

import numpy as np
import pytest

import jpeg_fixtures as F
import mesh_points_fixtures as M
from opencalibration_amd import capi, host


def _seed(h, w):
    return h * 131 + w


def _pillow(rgb, quality=95, **how):
    Image = pytest.importorskip("PIL.Image")
    f = io.BytesIO()
    Image.fromarray(rgb).save(f, format="JPEG", quality=quality, **how)
    return f.getvalue()


# ----------------------------------------------------------------------------------------------------- the committed files
@pytest.mark.parametrize("case", F.GOLDEN, ids=F.golden_name)
def test_equals_the_committed_libjpeg_turbo_file(case):
    kind, h, w, q, seed = case
    assert host.encode_jpeg(F.content(kind, h, w, seed), quality=q) == F.golden_bytes(case)


def test_golden_noise_holds_stuffed_bytes():
    scan = F.scan_of(F.golden_bytes(("noise", 33, 47, 95, 5)))
    assert scan.count(b"\xff\x00") == 20 and b"\xff" not in scan.replace(b"\xff\x00", b"")


def test_golden_flat_is_the_hand_derived_scan():
    """16 x 16 of 255: Y DC 1016 / 8 = 127 -> category 7 (code 11110) and 1111111, EOB 1010; three Y blocks and two chroma
    blocks of difference 0 (00 / 00) and their EOBs (1010 / 00); 46 bits and two 1-bits of filling.  Every further MCU adds
    six zero differences and six EOBs: 32 bits."""
    assert F.scan_of(F.golden_bytes(("flat", 16, 16, 95, 0))) == F.FLAT_SCAN_16
    assert F.scan_of(F.golden_bytes(("flat", 48, 64, 95, 0))) == F.FLAT_SCAN_16[:5] + b"\x00" + bytes.fromhex("a28a2800") * 10 + \
        bytes.fromhex("a28a2803")


def test_golden_checker_holds_zrl_symbols_at_quality_50():
    assert F.zrl_symbols(F.golden_bytes(("checker", 32, 48, 50, 0))) == 24
    assert F.zrl_symbols(host.encode_jpeg(F.checker(32, 48), quality=95)) == 0


# ------------------------------------------------------------------------------------------------------------ live Pillow
@pytest.mark.parametrize("shape", F.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_and_contents_equal_pillow(shape):
    h, w = shape
    for kind in F.CONTENTS:
        rgb = F.content(kind, h, w, _seed(h, w))
        assert host.encode_jpeg(rgb) == _pillow(rgb, subsampling=2, optimize=False), kind


@pytest.mark.parametrize("quality", F.QUALITIES)
def test_qualities_equal_pillow(quality):
    for h, w in F.QUALITY_SHAPES:
        for kind in ("noise", "ramp"):
            rgb = F.content(kind, h, w, _seed(h, w))
            assert host.encode_jpeg(rgb, quality=quality) == _pillow(rgb, quality, subsampling=2, optimize=False), (h, w, kind)


def test_pillows_default_subsampling_is_the_explicit_one():
    rgb = F.noise(33, 47, 5)
    assert _pillow(rgb) == _pillow(rgb, subsampling=2, optimize=False) == host.encode_jpeg(rgb)


# ----------------------------------------------------------------------------------------------------------- the encoder
def _fed(rgb, step, collect=True, quality=95):
    h, w = rgb.shape[:2]
    parts = []
    with host.JpegEncoder(w, h, quality=quality) as e:
        for r in range(0, h, step):
            e.feed(r, rgb[r:r + step])
            if collect:
                parts.append(e.collect())
        parts.append(e.finish())
    return parts


@pytest.mark.parametrize("shape", [(33, 47), (64, 80), (131, 23)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_any_split_of_the_rows_gives_the_same_bytes(shape):
    h, w = shape
    rgb = F.noise(h, w, _seed(h, w))
    whole = host.encode_jpeg(rgb)
    for step in (1, 7, 16, 17, h):
        parts = _fed(rgb, step)
        assert b"".join(parts) == whole, step            # collect at every step concatenates to the one-shot result
        assert b"".join(_fed(rgb, step, collect=False)) == whole, step
    assert _fed(rgb, 16)[0].startswith(b"\xff\xd8\xff\xe0") and _fed(rgb, 16)[-1].endswith(b"\xff\xd9")


def test_rgb_and_rgba_input_are_equal():
    for h, w in ((17, 33), (48, 64)):
        rgb = F.noise(h, w, 3)
        assert host.encode_jpeg(F.rgba_of(rgb)) == host.encode_jpeg(rgb)
        with host.JpegEncoder(w, h) as e:                  # and the two may alternate from band to band
            e.feed(0, rgb[:5])
            e.feed(5, F.rgba_of(rgb)[5:])
            assert e.collect() + e.finish() == host.encode_jpeg(rgb)


def test_refusals():
    for w, h, q, text in ((0, 4, 95, "a raster of 0 x 4"), (4, 0, 95, "a raster of 4 x 0"), (65501, 4, 95, "a raster of 65501 x 4"),
                          (4, 65501, 95, "a raster of 4 x 65501"), (4, 4, 0, "quality 0"), (4, 4, 101, "quality 101")):
        with pytest.raises(capi.OchipError, match=text):
            host.JpegEncoder(w, h, quality=q)
    rgb = F.ramp(40, 24)
    with host.JpegEncoder(24, 40) as e:
        with pytest.raises(capi.OchipError, match="gap: rows 8 to 16 when row 0 is next"):
            e.feed(8, rgb[8:16])
        e.feed(0, rgb[:20])
        with pytest.raises(capi.OchipError, match="overlap: rows 16 to 24 when row 20 is next"):
            e.feed(16, rgb[16:24])
        with pytest.raises(capi.OchipError, match="rows 20 to 60 of a raster of 40 rows"):
            e.feed(20, np.concatenate([rgb[20:], rgb[20:]]))
        with pytest.raises(capi.OchipError, match="finish at row 20 of 40"):
            e.finish()
        assert e.pending() > 600
        with pytest.raises(capi.OchipError, match="the capacity is 5"):
            e.collect(5)
        e.feed(20, rgb[20:])
        assert e.collect() + e.finish() == host.encode_jpeg(rgb)     # the refusals changed nothing
        with pytest.raises(capi.OchipError, match="after finish"):
            e.feed(40, rgb[:1])
        with pytest.raises(capi.OchipError, match="finish after finish"):
            e.finish()
        dead = e.h
    L = host.load()
    assert L.och_jpeg_feed(dead, 0, 1, rgb.ctypes.data, 3, 0) == -1    # OCHIP_EINVAL: a dead handle is refused, not followed
    assert "not a live" in L.och_jpeg_last_error().decode()
    assert L.och_jpeg_finish(dead) == -1 and L.och_jpeg_pending(dead) == 0
    with pytest.raises(ValueError):
        host.JpegEncoder(4, 4, on_device=True)
    with host.JpegEncoder(4, 4) as e:
        with pytest.raises(ValueError):
            e.feed(0, np.zeros((4, 5, 3), np.uint8))
        with pytest.raises(ValueError):
            e.feed(0, np.zeros((4, 4, 2), np.uint8))


# ---------------------------------------------------------------------------------------------------- the textured OBJ
GEOMETRY = (64, 48, -12.5, 83.25, 0.0371, 0.0371)


def _site():
    plan = dict(width=GEOMETRY[0], height=GEOMETRY[1], gsd=GEOMETRY[4], min_x=GEOMETRY[2], max_x=-10.1256, min_y=81.4692,
                max_y=GEOMETRY[3], mean_camera_z=50.0)
    rgba = np.random.default_rng(0).integers(0, 256, (plan["height"], plan["width"], 4), dtype=np.uint8)
    return [M.mesh("minimal")], plan, rgba


def test_save_textured_obj_writes_the_jpeg_the_mtl_names(tmp_path):
    surfaces, plan, rgba = _site()
    data = host.save_textured_obj(tmp_path / "site.obj", surfaces, rgba, plan, jpeg=True)
    assert sorted(os.listdir(tmp_path)) == ["site.jpg", "site.mtl", "site.obj"]
    assert (tmp_path / "site.jpg").read_bytes() == data == host.encode_jpeg(rgba)
    named = [l.split()[1] for l in (tmp_path / "site.mtl").read_bytes().split(b"\n") if l.startswith(b"map_Kd ")]
    assert named == [b"site.jpg"]
    obj, mtl, jpg = host.save_textured_obj(None, surfaces, rgba, plan, jpeg=True, quality=50)
    assert (obj, mtl) == host.textured_obj(surfaces, plan, "model") and jpg == host.encode_jpeg(rgba[:, :, :3], quality=50)
    Image = pytest.importorskip("PIL.Image")
    with Image.open(tmp_path / "site.jpg") as im:
        assert im.size == (plan["width"], plan["height"]) and im.mode == "RGB"
        im.load()                                                                 # the whole scan decodes


def test_save_textured_obj_without_jpeg_is_unchanged(tmp_path):
    surfaces, plan, rgba = _site()
    texture = host.save_textured_obj(tmp_path / "site.obj", surfaces, rgba, plan)
    assert isinstance(texture, np.ndarray) and np.array_equal(texture, rgba[:, :, :3])
    assert sorted(os.listdir(tmp_path)) == ["site.mtl", "site.obj"]
    obj, mtl = host.textured_obj(surfaces, plan, "site")
    assert (tmp_path / "site.obj").read_bytes() == obj and (tmp_path / "site.mtl").read_bytes() == mtl
    obj, mtl, tex = host.save_textured_obj(None, surfaces, rgba, plan)
    assert (obj, mtl) == host.textured_obj(surfaces, plan, "model") and np.array_equal(tex, rgba[:, :, :3])
