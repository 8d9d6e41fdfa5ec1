"""The per-tile progress thumbnails on the CPU route (csrc/host/ortho_tile_thumbs.cpp, csrc/ortho_tile_thumbs.hpp; DESIGN.md
§4.15) against the yardstick of tile_progress_fixtures.py - the reference's two loops restated in numpy - bit for bit: every
shape with every layer count and content, the thumbnail geometry, the records over a raster fed in two bands, the slots'
zero padding, and the refusals."""
import ctypes

import numpy as np
import pytest

from opencalibration_amd import capi, host
from tile_progress_fixtures import (BACKGROUND_ALPHA, BLEND_CONTENTS, CASES, LAYER_CONTENTS, LAYER_COUNTS, blended, case_id,
                                    difference, layers, mosaic_difference, mosaic_order, mosaic_plan, plan_of, slots_of,
                                    thumb_dims, yardstick)


@pytest.mark.parametrize("num_layers", LAYER_COUNTS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_layer_pass_equals_the_yardstick(case, num_layers):
    cols, rows, t = case
    plan = plan_of(cols, rows)
    for content in LAYER_CONTENTS:
        bgra, weight = layers(content, num_layers, rows, cols)
        got = host.ortho_tile_updates(plan, bgra, 1, tile_size=t, weight=weight)
        assert difference(got, yardstick(plan, bgra, 1, t, weight=weight)) == "", content


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_blend_pass_equals_the_yardstick(case):
    cols, rows, t = case
    plan = plan_of(cols, rows)
    for content in BLEND_CONTENTS:
        rgba = blended(content, rows, cols)
        got = host.ortho_tile_updates(plan, rgba, 2, tile_size=t)
        assert difference(got, yardstick(plan, rgba, 2, t)) == "", content


def test_contents_reach_the_cases_they_are_for():
    plan, t = plan_of(300, 130), 128

    def thumbs(content, num_layers):
        bgra, weight = layers(content, num_layers, 130, 300)
        return bgra, weight, np.concatenate([u["thumbnail"].reshape(-1, 4) for u in yardstick(plan, bgra, 1, t, weight=weight)])

    for content in ("all_invalid", "nan_alone", "weight_minus_half"):  # background everywhere, colour zero
        assert (thumbs(content, 2)[2] == (0, 0, 0, BACKGROUND_ALPHA)).all(), content
    assert BACKGROUND_ALPHA == 51
    bgra, _, got = thumbs("only_layer_1", 2)
    assert set(np.unique(got[:, 3])) == {BACKGROUND_ALPHA, 255}
    bgra, _, got = thumbs("equal_weights", 8)  # the lower layer's colour: the first tile's first row is raster row 0
    assert np.array_equal(got[:128, :3], bgra[0, 0, :128, :3]) and not np.array_equal(got[:128, :3], bgra[7, 0, :128, :3])
    bgra, _, got = thumbs("heavier_upper", 8)
    assert np.array_equal(got[:128, :3], bgra[7, 0, :128, :3])
    bgra, _, got = thumbs("weight_zero", 2)  # a weight of 0 is a hit: best >= 0
    assert (got[:, 3] == 255).all() and np.array_equal(got[:128, :3], bgra[0, 0, :128, :3])
    bgra, weight, got = thumbs("nan_beside_finite", 2)  # the finite layer wins, whichever side the NaN is on
    assert (got[:, 3] == 255).all()
    finite_first = ~np.isnan(weight[0, 0, :128])
    assert finite_first.any() and (~finite_first).any()
    assert np.array_equal(got[:128, :3], np.where(finite_first[:, None], bgra[0, 0, :128, :3], bgra[1, 0, :128, :3]))
    grey = np.concatenate([u["thumbnail"].reshape(-1, 4) for u in yardstick(plan, blended("alpha_0_grey", 130, 300), 2, t)])
    assert (grey == 0).all()
    one = blended("alpha_1", 130, 300)
    got = yardstick(plan, one, 2, t)[0]["thumbnail"]
    assert (got[..., 3] == 255).all() and np.array_equal(got[0, :, :3], one[0, :128, [2, 1, 0]].T)


def test_thumb_dims():
    sizes = sorted(set(range(1, 301)) | {p + d for p in (1 << k for k in range(13)) for d in (-1, 0, 1) if 1 <= p + d <= 4096})
    L = capi.load()
    dims = np.zeros(3, np.int32)
    for tw in sizes:
        for th in sizes:
            assert L.ochip_ortho_tile_thumb_dims(tw, th, dims.ctypes.data) == 0
            assert tuple(dims) == thumb_dims(tw, th), (tw, th)
    assert host.tile_thumb_dims(1024, 76) == (8, 128, 10) and host.tile_thumb_dims(6, 76) == (1, 6, 76)
    assert host.tile_thumb_dims(4096, 4096) == (32, 128, 128) and host.tile_thumb_dims(129, 1) == (2, 65, 1)
    for tw, th in ((0, 5), (5, 0), (4097, 1), (1, 4097)):
        with pytest.raises(ValueError):
            host.tile_thumb_dims(tw, th)
    assert L.ochip_ortho_tile_thumb_dims(5, 5, None) == -1


def test_records_over_a_raster_fed_in_two_bands():
    """3 x 2 tiles of 32 over 70 x 40: a band of one whole tile row, then the 8 rows left"""
    plan, t = plan_of(70, 40), 32
    bgra, weight = layers("mixed", 2, 40, 70)
    rgba = blended("alpha_mixed", 40, 70)
    with host.TileProgress(plan, t, 2) as p:
        p.feed(1, 0, bgra[:, :32], weight[:, :32])
        p.feed(2, 0, rgba[:32])
        p.feed(1, 32, bgra[:, 32:], weight[:, 32:])
        assert p.pending() == 3
        first = p.collect()
        assert p.pending() == 2
        p.feed(2, 32, rgba[32:])
        got = [first, p.collect(), p.collect(), p.collect()]
        assert p.pending() == 0
        with pytest.raises(capi.OchipError, match="no band is pending"):
            p.collect()
    want = [yardstick(plan, bgra[:, :32], 1, t, 0, weight[:, :32]), yardstick(plan, rgba[:32], 2, t, 0),
            yardstick(plan, bgra[:, 32:], 1, t, 32, weight[:, 32:]), yardstick(plan, rgba[32:], 2, t, 32)]
    for g, x in zip(got, want):
        assert difference(g, x) == ""
    assert [u["tile_index"] for u in got[0] + got[2]] == [1, 2, 3, 4, 5, 6]
    assert [u["tile_index"] for u in got[1] + got[3]] == [1, 2, 3, 4, 5, 6]
    last = got[3][2]
    assert {k: last[k] for k in ("pixel_x", "pixel_y", "pixel_w", "pixel_h", "total_output_width", "total_output_height",
                                 "total_tiles", "thumb_w", "thumb_h", "scale", "pass")} == \
        dict(pixel_x=64, pixel_y=32, pixel_w=6, pixel_h=8, total_output_width=70, total_output_height=40, total_tiles=6,
             thumb_w=6, thumb_h=8, scale=1) | {"pass": 2}
    assert (last["bounds_min_x"], last["bounds_max_y"], last["meters_per_pixel"]) == (plan["min_x"], plan["max_y"], plan["gsd"])
    # one band from the middle of a raster: ortho_tile_updates' row0
    assert difference(host.ortho_tile_updates(plan, rgba[32:], 2, row0=32, tile_size=t), want[3]) == ""
    assert host.TILE_UPDATE_DTYPE.itemsize == 72


@pytest.mark.parametrize("case", [(300, 130, 128), (260, 129, 129), (70, 40, 32), (1, 1, 1)], ids=case_id)
def test_slot_padding_is_zero(case):
    cols, rows, t = case
    plan = plan_of(cols, rows)
    bgra, weight = layers("weight_zero", 2, rows, cols)  # every thumbnail pixel has alpha 255: only the padding is zero
    for pass_, pixels, w in ((1, bgra, weight), (2, blended("alpha_1", rows, cols), None)):
        want = slots_of(yardstick(plan, pixels, pass_, t, weight=w), t)
        raw = host.ortho_tile_thumbs(pixels, pass_, tile_size=t, weight=w)
        assert raw.shape == want.shape == (-(-cols // t) * -(-rows // t), min(t, 128) ** 2, 4)
        assert np.array_equal(raw, want)
        with host.TileProgress(plan, t, 2) as p:
            p.feed(pass_, 0, pixels, w)
            records, slots = p.collect(raw=True)
        assert np.array_equal(slots, want)
        for r, slot in zip(records, slots):
            n = int(r["thumb_w"]) * int(r["thumb_h"])
            assert (slot[:n, 3] == 255).all() and (slot[n:] == 0).all()
    if case == (300, 130, 128):
        assert [(int(r["thumb_w"]), int(r["thumb_h"])) for r in records] == [(128, 128), (128, 128), (44, 128), (128, 2), (128, 2), (44, 2)]


def test_refusals():
    L = capi.load()
    px = np.zeros((2, 8, 8, 4), np.uint8)
    wt = np.zeros((2, 8, 8), np.float32)
    out = np.zeros((1, 64, 4), np.uint8)

    def call(pass_=1, cols=8, rows=8, t=8, nl=2, on_device=0, pixels=px.ctypes.data, weight=wt.ctypes.data, thumbs=out.ctypes.data):
        rc = L.ochip_ortho_tile_thumbs(None, pass_, cols, rows, t, nl, on_device, pixels, weight, thumbs)
        return rc, L.ochip_last_error(None).decode()

    assert call()[0] == 0
    for kwargs, text in ((dict(pass_=0), "pass 0"), (dict(pass_=3), "pass 3"), (dict(t=0), "tile_size 0"), (dict(t=4097), "tile_size 4097"),
                         (dict(nl=0), "num_layers 0"), (dict(nl=9), "num_layers 9"), (dict(cols=0), "0 x 8"), (dict(cols=-1), "-1 x 8"),
                         (dict(rows=0), "8 x 0"), (dict(rows=-5), "8 x -5"), (dict(pixels=None), "pixels are NULL"),
                         (dict(weight=None), "needs the layers' weights"), (dict(thumbs=None), "thumbnails' array is NULL"),
                         (dict(pixels=px.ctypes.data + 1), "aligned"), (dict(on_device=1), "device context")):
        rc, message = call(**kwargs)
        assert rc == -1 and text in message, (kwargs, rc, message)
    assert call(pass_=2, weight=None, nl=1)[0] == 0  # the blend pass reads no weights
    # the object: its own arguments, then the rows
    H = host.load()
    h = ctypes.c_void_p()
    plan8 = host._plan_array(plan_of(70, 40))
    for t, nl in ((0, 2), (4097, 2), (32, 0), (32, 9)):
        assert H.och_tile_progress_create(None, plan8, t, nl, ctypes.byref(h)) == -1 and not h.value
        assert b"tile_size" in H.och_tile_progress_last_error()
    assert H.och_tile_progress_create(None, host._plan_array(plan_of(0, 40)), 32, 2, ctypes.byref(h)) == -1
    assert H.och_tile_progress_feed(None, 1, 0, 8, 0, px.ctypes.data, wt.ctypes.data) == -1
    bgra, weight = layers("mixed", 2, 40, 70)
    rgba = blended("alpha_mixed", 40, 70)
    with host.TileProgress(plan_of(70, 40), 32, 2) as p:
        with pytest.raises(capi.OchipError, match=r"rows 16 to 40: row 16 is not on a tile row \(tile_size 32\)"):
            p.feed(2, 16, rgba[16:])
        with pytest.raises(capi.OchipError, match=r"gap: rows 32 to 40 of pass 2 when row 0 is next"):
            p.feed(2, 32, rgba[32:])
        with pytest.raises(capi.OchipError, match=r"rows 0 to 20 are neither whole tile rows"):
            p.feed(2, 0, rgba[:20])
        with pytest.raises(capi.OchipError, match=r"rows 0 to 64 of a raster of 40 rows"):
            p.feed(2, 0, np.concatenate([rgba, rgba[:24]]))
        with pytest.raises(capi.OchipError, match="needs the layers' weights"):
            p.feed(1, 0, bgra[:, :32])
        with pytest.raises(capi.OchipError, match="pass 3"):
            p.feed(3, 0, rgba[:32])
        assert p.pending() == 0  # a refused feed changes nothing
        p.feed(2, 0, rgba[:32])
        with pytest.raises(capi.OchipError, match=r"out of raster order: rows 0 to 32 of pass 2 when row 32 is next"):
            p.feed(2, 0, rgba[:32])
        p.feed(1, 0, bgra[:, :32], weight[:, :32])  # the passes keep their own order
        p.feed(2, 32, rgba[32:])
        p.feed(2, 0, rgba[:32])  # after the last row a pass may start again
        n = ctypes.c_uint64(0)
        records = np.zeros(3, host.TILE_UPDATE_DTYPE)
        slots = np.zeros((3, 32 * 32, 4), np.uint8)
        assert H.och_tile_progress_collect(p.h, records.ctypes.data, slots.ctypes.data, 2, ctypes.byref(n)) == -1 and n.value == 3
        assert b"3 tiles, the capacity is 2" in H.och_tile_progress_last_error() and p.pending() == 4
        assert H.och_tile_progress_collect(p.h, records.ctypes.data, None, 3, ctypes.byref(n)) == -1 and p.pending() == 4
        assert len(p.collect()) == 3 and p.pending() == 3
    with pytest.raises(ValueError):
        host.ortho_tile_updates(plan_of(8, 8), np.zeros((8, 8, 3), np.uint8), 2, tile_size=8)
    with pytest.raises(ValueError):
        host.ortho_tile_updates(plan_of(8, 8), np.zeros((8, 8, 4), np.float32), 2, tile_size=8)
    with pytest.raises(ValueError):
        host.ortho_tile_updates(plan_of(9, 8), np.zeros((8, 8, 4), np.uint8), 2, tile_size=8)  # not the raster's width


def test_mosaic_cpu_route_emits_the_updates():
    """the CPU route of the mosaic on the four-camera scene (105 x 90, tiles of 32, bands of 64 and 26 rows): the raster is
    the one without progress, every update is delivered before return in the order stated, pass 2 equals the yardstick over
    the returned raster and pass 1 over ortho_layers_bands' outputs"""
    from layers_fixtures import four_camera_scene

    g, s, imgs = four_camera_scene(seed=4)
    plan = mosaic_plan(0.1)
    cfg = dict(tile_size=32, blend_transition_radius=10)
    plain = host.ortho_mosaic(plan, g, [s], imgs, config=cfg, tile_rows=2)
    got = []
    out = host.ortho_mosaic(plan, g, [s], imgs, config=cfg, tile_rows=2, progress=got.append)
    assert isinstance(out, np.ndarray) and np.array_equal(out, plain)
    bands = list(host.ortho_layers_bands(plan, g, [s], imgs, tile_rows=2, config=dict(tile_size=32)))
    assert mosaic_order(got, plan, 32, 2, solve=False) == ""
    assert mosaic_difference(got, plan, 32, out, bands) == ""
    only_blend = []
    host.ortho_mosaic(plan, g, [s], imgs, config=cfg, tile_rows=2, progress=only_blend.append, progress_passes=(2,))
    assert difference(only_blend, [u for u in got if u["pass"] == 2]) == ""
    solved = []
    out2 = host.ortho_mosaic(plan, g, [s], imgs, config=cfg, tile_rows=2, color_balance="solve", progress=solved.append)
    assert mosaic_order(solved, plan, 32, 2, solve=True) == ""
    assert mosaic_difference(solved, plan, 32, out2, bands) == ""

    def boom(update):
        raise RuntimeError("the callback's own")

    with pytest.raises(RuntimeError, match="the callback's own"):
        host.ortho_mosaic(plan, g, [s], imgs, config=cfg, tile_rows=2, progress=boom)
    with pytest.raises(ValueError):
        host.ortho_mosaic(plan, g, [s], imgs, config=cfg, tile_rows=2, progress=got.append, progress_passes=(3,))
    g.close()
