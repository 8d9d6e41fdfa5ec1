"""Shared by test_tile_progress_host.py and tile_progress_gpu_child.py: the shapes and contents of the tile-progress tests, and
the yardstick - the two thumbnail loops of the reference (generateLayeredGeoTIFF, src/ortho/ortho.cpp:1553-1614, and
blendLayeredGeoTIFF, :1962-2011) restated in plain numpy, with the TileUpdate record around them.  Nothing here goes through
the library."""
import numpy as np

# (cols, rows, tile_size): one tile of one pixel; a partial column and row of tiles at the 128 threshold; a tile size just
# above it (scale 2) with 2- and 1-pixel leftovers; three sizes around 256; the default size with a 76-column and a 6-row
# leftover; one 4096 tile (scale 32) with a 4-column one beside it
CASES = [(1, 1, 1), (300, 130, 128), (260, 129, 129), (520, 300, 255), (520, 300, 256), (520, 300, 257), (1100, 1030, 1024),
         (4100, 200, 4096)]
LAYER_COUNTS = (1, 2, 8)
LAYER_CONTENTS = ["all_invalid", "only_layer_1", "equal_weights", "heavier_upper", "weight_zero", "nan_alone",
                  "nan_beside_finite", "weight_minus_half", "mixed"]
BLEND_CONTENTS = ["alpha_0_grey", "alpha_1", "alpha_mixed"]
BACKGROUND_ALPHA = 255 * 20 // 100
FIELDS = ("pixel_x", "pixel_y", "pixel_w", "pixel_h", "total_output_width", "total_output_height", "tile_index", "total_tiles",
          "thumb_w", "thumb_h", "scale", "pass", "bounds_min_x", "bounds_max_y", "meters_per_pixel")


def case_id(case):
    return f"{case[0]}x{case[1]}_T{case[2]}"


def plan_of(cols, rows):
    return dict(width=cols, height=rows, gsd=0.125, min_x=-3.5, max_x=-3.5 + cols * 0.125, min_y=2.25 - rows * 0.125, max_y=2.25,
                mean_camera_z=40.0)


def _seed(content, *shape):
    return sum(map(ord, content)) * 1000003 + sum(int(v) * 1009 ** i for i, v in enumerate(shape))


def layers(content, num_layers, rows, cols):
    """(bgra (L, rows, cols, 4) uint8, weight (L, rows, cols) float32) of a pass-1 content"""
    rng = np.random.default_rng(_seed(content, num_layers, rows, cols))
    shape = (num_layers, rows, cols)
    bgra = rng.integers(1, 256, shape + (4,), dtype=np.uint8)  # alpha 1 .. 255: valid
    weight = rng.uniform(0.001, 2.0, shape).astype(np.float32)
    if content == "all_invalid":
        bgra[..., 3] = 0
    elif content == "only_layer_1":  # the second layer alone (the only one there is when L = 1), on half of the pixels
        only = min(1, num_layers - 1)
        alpha = np.where(rng.random((rows, cols)) < 0.5, bgra[only, ..., 3], 0)
        bgra[..., 3] = 0
        bgra[only, ..., 3] = alpha
    elif content == "equal_weights":  # the first and the last layer share the greatest weight: the lower one is kept
        weight[0] = weight[-1] = np.float32(3.0)
    elif content == "heavier_upper":
        weight[:] = np.sort(weight, axis=0)
    elif content == "weight_zero":
        weight[:] = 0
    elif content == "nan_alone":
        weight[:] = np.nan
    elif content == "nan_beside_finite":  # the NaN in the first layer on one half, in the last on the other
        first = rng.random((rows, cols)) < 0.5
        weight[0][first] = np.nan
        weight[-1][~first] = np.nan
    elif content == "weight_minus_half":
        weight[:] = -0.5
    elif content == "mixed":
        bgra[..., 3] = rng.choice(np.array([0, 0, 1, 255], np.uint8), shape)
        weight = rng.choice(np.array([np.nan, -0.5, -0.0, 0.0, 0.0005, 1.0, 1.0, 2.5, np.inf], np.float32), shape)
    else:
        raise KeyError(content)
    return bgra, weight


def blended(content, rows, cols):
    """rgba (rows, cols, 4) uint8 of a pass-2 content"""
    rng = np.random.default_rng(_seed(content, rows, cols))
    rgba = rng.integers(1, 256, (rows, cols, 4), dtype=np.uint8)
    if content == "alpha_0_grey":  # the blend's checkerboard where no layer is valid
        yy, xx = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
        rgba[..., :3] = np.where((yy // 8 + xx // 8) % 2 == 0, 64, 128)[..., None]
        rgba[..., 3] = 0
    elif content == "alpha_1":
        rgba[..., 3] = 1
    elif content == "alpha_mixed":
        rgba[..., 3] = rng.choice(np.array([0, 1, 128, 255], np.uint8), (rows, cols))
    else:
        raise KeyError(content)
    return rgba


def thumb_dims(tw, th):
    scale = max(1, (max(tw, th) + 127) // 128)
    return scale, (tw + scale - 1) // scale, (th + scale - 1) // scale


def _sampled(tile, tw, th):
    """the tile's pixels a thumbnail reads: (..., thumb_h, thumb_w) + the tile's trailing axes"""
    scale, thumb_w, thumb_h = thumb_dims(tw, th)
    rr = np.minimum(np.arange(thumb_h) * scale, th - 1)
    cc = np.minimum(np.arange(thumb_w) * scale, tw - 1)
    return tile[rr][:, cc]


def layer_thumbnail(bgra_tile, weight_tile):
    """the loop of ortho.cpp:1572-1597 over one tile: bgra (L, th, tw, 4), weight (L, th, tw) -> BGRA (thumb_h, thumb_w, 4)"""
    num_layers, th, tw = weight_tile.shape
    scale, thumb_w, thumb_h = thumb_dims(tw, th)
    out = np.zeros((thumb_h, thumb_w, 4), np.uint8)
    out[..., 3] = BACKGROUND_ALPHA
    best_weight = np.full((thumb_h, thumb_w), -1.0, np.float32)
    best_color = np.zeros((thumb_h, thumb_w, 3), np.uint8)
    for layer in range(num_layers):
        sample = _sampled(bgra_tile[layer], tw, th)
        weight = _sampled(weight_tile[layer], tw, th)
        with np.errstate(invalid="ignore"):
            take = (sample[..., 3] > 0) & (weight > best_weight)
        best_weight = np.where(take, weight, best_weight)
        best_color = np.where(take[..., None], sample[..., :3], best_color)
    with np.errstate(invalid="ignore"):
        hit = best_weight >= np.float32(0)
    out[..., :3] = np.where(hit[..., None], best_color, 0)
    out[..., 3] = np.where(hit, 255, BACKGROUND_ALPHA)
    return out


def blend_thumbnail(rgba_tile):
    """the loop of ortho.cpp:1978-1994 over one tile: rgba (th, tw, 4) -> BGRA (thumb_h, thumb_w, 4)"""
    th, tw = rgba_tile.shape[:2]
    sample = _sampled(rgba_tile, tw, th)
    out = np.zeros(sample.shape, np.uint8)
    hit = sample[..., 3] > 0
    out[..., 0] = np.where(hit, sample[..., 2], 0)
    out[..., 1] = np.where(hit, sample[..., 1], 0)
    out[..., 2] = np.where(hit, sample[..., 0], 0)
    out[..., 3] = np.where(hit, 255, 0)
    return out


def yardstick(plan, pixels, pass_, tile_size, row0=0, weight=None):
    """the updates of one band: the reference's tile loop, tiles row-major, tile_index over the whole raster"""
    pixels = np.asarray(pixels)
    rows = pixels.shape[-3]
    width, height, t = plan["width"], plan["height"], tile_size
    tiles_x, tiles_y = -(-width // t), -(-height // t)
    updates = []
    for ty in range(-(-rows // t)):
        for tx in range(tiles_x):
            x_off, y_off = tx * t, ty * t
            tw, th = min(t, width - x_off), min(t, rows - y_off)
            if pass_ == 1:
                thumb = layer_thumbnail(pixels[:, y_off:y_off + th, x_off:x_off + tw], np.asarray(weight)[:, y_off:y_off + th, x_off:x_off + tw])
            else:
                thumb = blend_thumbnail(pixels[y_off:y_off + th, x_off:x_off + tw])
            scale, thumb_w, thumb_h = thumb_dims(tw, th)
            updates.append({"pixel_x": x_off, "pixel_y": row0 + y_off, "pixel_w": tw, "pixel_h": th, "total_output_width": width,
                            "total_output_height": height, "tile_index": (row0 // t + ty) * tiles_x + tx + 1,
                            "total_tiles": tiles_x * tiles_y, "thumb_w": thumb_w, "thumb_h": thumb_h, "scale": scale, "pass": pass_,
                            "bounds_min_x": plan["min_x"], "bounds_max_y": plan["max_y"], "meters_per_pixel": plan["gsd"],
                            "thumbnail": thumb})
    return updates


def difference(got, want):
    """"" when two lists of updates are equal, field for field and thumbnail for thumbnail; else what differs first"""
    if len(got) != len(want):
        return f"{len(got)} updates, {len(want)} expected"
    for i, (g, x) in enumerate(zip(got, want)):
        for k in FIELDS:
            if g[k] != x[k]:
                return f"update {i}: {k} is {g[k]!r}, expected {x[k]!r}"
        a, b = g["thumbnail"], x["thumbnail"]
        if a.shape != b.shape or a.dtype != np.uint8:
            return f"update {i}: a thumbnail of {a.shape} {a.dtype}, expected {b.shape}"
        if not np.array_equal(a, b):
            return f"update {i} (tile_index {x['tile_index']}): {int((a != b).any(axis=-1).sum())} of {a.shape[0] * a.shape[1]} pixels differ"
    return ""


def slots_of(updates, tile_size):
    """the raw slots the updates' thumbnails fill: (tiles, min(T, 128)^2, 4), zeros behind each thumbnail"""
    side = min(tile_size, 128)
    out = np.zeros((len(updates), side * side, 4), np.uint8)
    for slot, u in zip(out, updates):
        slot[:u["thumb_w"] * u["thumb_h"]] = u["thumbnail"].reshape(-1, 4)
    return out


def mosaic_plan(gsd):
    """the raster of the four-camera scene (layers_fixtures.four_camera_scene): 105 x 90 at 0.1, 210 x 180 at 0.05"""
    return dict(width=int(10.5 / gsd), height=int(9.0 / gsd), gsd=gsd, min_x=-2.0, max_x=8.5, min_y=-2.0, max_y=7.0,
                mean_camera_z=10.0)


def mosaic_order(updates, plan, tile_size, tile_rows, solve):
    """"" when a mosaic's updates came in the stated order: with "solve" all of pass 1 and then all of pass 2, otherwise
    band by band a band's pass-1 tiles and then its pass-2 tiles; within a pass in tile_index order, every tile once"""
    tiles_x, tiles_y = -(-plan["width"] // tile_size), -(-plan["height"] // tile_size)
    got = [(u["pass"], u["tile_index"]) for u in updates]
    every = list(range(1, tiles_x * tiles_y + 1))
    if solve:
        want = [(1, i) for i in every] + [(2, i) for i in every]
    else:
        want = []
        for first in range(0, tiles_y, tile_rows):
            band = [i for i in every if first * tiles_x < i <= min(first + tile_rows, tiles_y) * tiles_x]
            want += [(1, i) for i in band] + [(2, i) for i in band]
    return "" if got == want else f"order {got}, expected {want}"


def mosaic_difference(updates, plan, tile_size, raster, bands):
    """"" when a mosaic's pass-2 updates equal the yardstick over the returned raster and its pass-1 updates the yardstick
    over the layered bands (ortho_layers' results as numpy: bgra, weight, row0)"""
    want1 = []
    for b in bands:
        want1 += yardstick(plan, np.asarray(b["bgra"]), 1, tile_size, int(b["row0"]), np.asarray(b["weight"]))
    d = difference([u for u in updates if u["pass"] == 1], want1)
    if d:
        return "pass 1: " + d
    d = difference([u for u in updates if u["pass"] == 2], yardstick(plan, np.asarray(raster), 2, tile_size))
    return "pass 2: " + d if d else ""
