"""Scenes and restatements for the streamed layered render's tests (test_ortho_stream_host.py, ortho_stream_gpu_child.py):
the band-set scenes, the strip scene whose bands read different cameras, the per-band union of the render's own kNN, and
the residency rule of csrc/host/ortho_residency.hpp restated in Python with a simulator of its invariants."""
import numpy as np

from layers_fixtures import DISTORTED, four_camera_scene, noise_images
from ortho_fixtures import DOWN, cloud_surface, jittered_cameras, make_graph, qmul, quat
from opencalibration_amd import host

AHEAD, LATE = host.LOAD_AHEAD, host.LOAD_LATE


def _flat_scene(pos, ori, seed, n_images=None):
    pos = np.asarray(pos, np.float64)
    g = make_graph(pos, ori, DISTORTED)
    lo, hi = pos[:, :2].min(0) - 6, pos[:, :2].max(0) + 6
    pts = cloud_surface([(lo[0], lo[1], 0), (hi[0], lo[1], 0), (hi[0], hi[1], 0), (lo[0], hi[1], 0),
                         ((lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2, 0.5)])
    s = host.rebuild_mesh(pos, previous=pts)
    return g, s, noise_images(len(pos) if n_images is None else n_images, 120, 160, seed)


def plan_of(width, height, gsd, min_x, max_y, mean_camera_z=10.0):
    return dict(width=width, height=height, gsd=gsd, min_x=min_x, max_x=min_x + width * gsd, min_y=max_y - height * gsd,
                max_y=max_y, mean_camera_z=mean_camera_z)


def scene_four_cameras():
    """fewer than 5 cameras: every kNN list keeps NONE entries"""
    g, s, imgs = four_camera_scene()
    return g, s, imgs, plan_of(105, 90, 0.1, -2.0, 7.0), dict(tile_size=32)


def scene_33_cameras():
    """a camera table whose tail is no multiple of 32 (nor of the workgroup's 256)"""
    pos, ori = jittered_cameras(11, 3, spacing=4.0, height=10.0, seed=5)
    g, s, imgs = _flat_scene(pos, ori, 6)
    return g, s, imgs, plan_of(120, 80, 0.4, -3.0, 13.0), dict(tile_size=16)


def scene_partial_tiles():
    """70 x 45 pixels in 16-row bands: a partial last 16 x 16 tile in both axes and a partial last band"""
    pos, ori = jittered_cameras(4, 3, spacing=5.0, height=10.0, seed=7)
    g, s, imgs = _flat_scene(pos, ori, 8)
    return g, s, imgs, plan_of(70, 45, 0.3, -2.0, 12.0), dict(tile_size=16)


def scene_exact_ties():
    """cameras on an integer lattice 4 m apart, min_x 0, max_y 40, gsd 0.5: every coordinate and squared distance is exact
    in fp64; pixel centres at x = 2, 6, ... are equidistant from two cameras, lattice centres from four"""
    pos = [(4.0 * i, 12.0 + 4.0 * j, 10.0) for j in range(8) for i in range(7)]
    g, s, imgs = _flat_scene(pos, [DOWN] * len(pos), 9)
    return g, s, imgs, plan_of(48, 48, 0.5, 0.0, 40.0), dict(tile_size=16)


BAND_SET_SCENES = dict(four_cameras=scene_four_cameras, cameras_33=scene_33_cameras, partial_tiles=scene_partial_tiles,
                       exact_ties=scene_exact_ties)


def scene_overflow():
    """1 100 cameras, 1 030 of them at one XY with different heights: a tile's candidate list exceeds the kernel's 1 024
    and every pixel scans the whole table.  Camera records only (no graph): cams (n, 28) and a plan."""
    rng = np.random.default_rng(11)
    cams = np.zeros((1100, 28))
    cams[:70, :2] = rng.uniform(0, 20, (70, 2))
    cams[70:, :2] = (10.0, 10.0)
    cams[:, 2] = 10.0 + np.arange(1100) * 0.01
    order = rng.permutation(1100)
    return np.ascontiguousarray(cams[order]), plan_of(50, 40, 0.5, -2.0, 21.0)


def scene_knn_overflow():
    """1 040 cameras jittered inside the rectangle of pixel centres of the 16 x 16 tile (1, 1) of a 50 x 40 raster at gsd
    0.5, and 40 spread around it: that tile's candidate list exceeds the kernels' 1 024 and its pixels scan the whole table,
    the other tiles keep their lists.  Every camera shares one image."""
    rng = np.random.default_rng(13)
    plan = plan_of(50, 40, 0.5, -2.0, 21.0)
    x = np.arange(16, 32) * plan["gsd"] + plan["min_x"]
    y = plan["max_y"] - np.arange(16, 32) * plan["gsd"]
    inside = np.stack([rng.uniform(x[0] + 0.1, x[-1] - 0.1, 1040), rng.uniform(y[-1] + 0.1, y[0] - 0.1, 1040)], 1)
    around = np.stack([rng.uniform(-2, 23, 40), rng.uniform(1, 21, 40)], 1)
    pos = np.concatenate([inside, around])[rng.permutation(1080)]
    pos = np.concatenate([pos, 10.0 + rng.uniform(-0.3, 0.3, (1080, 1))], 1)
    held = (pos[:, 0] >= x[0]) & (pos[:, 0] <= x[-1]) & (pos[:, 1] >= y[-1]) & (pos[:, 1] <= y[0])
    assert held.sum() > 1024 and len(np.unique(pos[held, :2], axis=0)) == held.sum()  # the scene cannot stop overflowing
    ori = [qmul(quat(rng.normal(size=3), 0.04), DOWN) for _ in pos]
    g, s, imgs = _flat_scene(pos, ori, 14, n_images=1)
    return g, s, imgs * len(pos), plan, dict(tile_size=16, correspondence_subsample=5)


def strip_scene(seed=3):
    """12 distorted cameras in a 6 x 2 layout, the long side along y, over a flat mesh, with distinct seeded noise images:
    bands of one 64-pixel tile row read different cameras, so a wrong or stale slot changes pixels"""
    rng = np.random.default_rng(seed)
    pos = np.array([(6.0 * x, 5.0 * y, 10.0) for y in range(6) for x in range(2)])
    pos += rng.uniform(-0.4, 0.4, pos.shape) * np.array([1, 1, 0.3])
    ori = [qmul(quat(rng.normal(size=3), 0.04), DOWN) for _ in pos]
    g, s, imgs = _flat_scene(pos, ori, seed + 1)
    cfg = dict(tile_size=64, correspondence_subsample=9)
    return g, s, imgs, plan_of(200, 580, 0.05, -2.0, 27.0), cfg


def knn_band_sets(knn, n_cams, band_rows):
    """the per-band union of a render's kNN lists (rows, cols, 5), NONE entries dropped: bool (n_bands, n_cams)"""
    n_bands = -(-knn.shape[0] // band_rows)
    used = np.zeros((n_bands, n_cams), bool)
    for b in range(n_bands):
        ids = np.unique(knn[b * band_rows:(b + 1) * band_rows])
        used[b, ids[ids != 0xFFFFFFFF]] = True
    return used


def knn_offer_sets(cams, plan, band_rows):
    """the project's kNN (ortho_geom.hpp's knn_offer: cameras offered in table order, a strict < at every step of the
    insertion, so an entry carried past an equal distance is dropped) over every pixel, in numpy: bool (n_bands, n_cams)"""
    h, w = plan["height"], plan["width"]
    x = (np.arange(w) * plan["gsd"] + plan["min_x"])[None, :] + np.zeros((h, 1))
    y = (plan["max_y"] - np.arange(h) * plan["gsd"])[:, None] + np.zeros((1, w))
    bd = np.full((5, h, w), np.inf)
    bi = np.full((5, h, w), -1, np.int64)
    for i, c in enumerate(cams):
        dx, dy = x - c[0], y - c[1]
        d, ident = dx * dx + dy * dy, np.full((h, w), i, np.int64)
        live = d < bd[4]
        for k in range(5):
            swap = live & (d < bd[k])
            bd[k], d = np.where(swap, d, bd[k]), np.where(swap, bd[k], d)
            bi[k], ident = np.where(swap, ident, bi[k]), np.where(swap, bi[k], ident)
    knn = np.where(bi < 0, 0xFFFFFFFF, bi).astype(np.uint32).transpose(1, 2, 0)
    return knn_band_sets(knn, len(cams), band_rows)


def band_cameras_raw(cams, plan, band_rows, ctx=None):
    """och_ortho_band_cameras over a bare camera table"""
    L = host.load()
    n_bands = -(-plan["height"] // band_rows)
    used = np.zeros((n_bands, len(cams)), np.uint8)
    raster4 = np.array([plan["min_x"], plan["max_y"], plan["gsd"], plan["mean_camera_z"]])
    rc = L.och_ortho_band_cameras(ctx.h if ctx is not None else None, raster4, plan["width"], plan["height"], band_rows, len(cams),
                                  cams.ctypes.data, used.ctypes.data)
    assert rc == 0, L.och_ortho_layers_last_error().decode()
    return used.astype(bool)


# ---- the residency rule restated (sets of cameras, a dict per slot) ----------------------------------------------------
def plan_restated(sets, capacity, resident=None):
    """sets: one set of cameras per band.  Returns (per band [(camera, slot, phase)], the slots' final state)."""
    slots = [-1] * capacity if resident is None else list(resident)
    out = []
    for k, cur in enumerate(sets):
        prev = sets[k - 1] if k else set()
        if len(cur) > capacity:
            raise ValueError(f"band {k} reads {len(cur)} images, the capacity is {capacity}")

        def next_use(cam):
            later = [j for j in range(k + 1, len(sets)) if cam in sets[j]]
            return later[0] if later else len(sets)

        loads = []
        for cam in sorted(cur):
            if cam in slots:
                continue
            free = [s for s in range(capacity) if slots[s] == -1]
            ahead = [s for s in range(capacity) if slots[s] != -1 and slots[s] not in cur and slots[s] not in prev]
            late = [s for s in range(capacity) if slots[s] != -1 and slots[s] not in cur]
            if free:
                slot, phase = free[0], AHEAD
            elif ahead:
                slot, phase = max(ahead, key=lambda s: (next_use(slots[s]), -s)), AHEAD
            else:
                slot, phase = max(late, key=lambda s: (next_use(slots[s]), -s)), LATE
            slots[slot] = cam
            loads.append((cam, slot, phase))
        out.append(loads)
    return out, slots


def simulate(sets, capacity, loads, resident=None):
    """replays the loads and checks the plan's invariants; returns the number of loads per camera"""
    slots = [-1] * capacity if resident is None else list(resident)
    count = {}
    for k, cur in enumerate(sets):
        prev = sets[k - 1] if k else set()
        for cam, slot, phase in loads[k]:
            assert 0 <= slot < capacity
            assert cam in cur and cam not in slots, "a load of a camera the band does not read, or that is resident"
            held = slots[slot]
            assert held not in cur, "a load evicts a camera of its own band"
            if phase == AHEAD:
                assert held not in prev, "an ahead load takes a slot the band that renders reads"
            else:
                assert phase == LATE
            slots[slot] = cam
            count[cam] = count.get(cam, 0) + 1
        assert cur <= set(slots), f"band {k} renders without {cur - set(slots)}"
    return count


def sets_of(used):
    return [set(np.nonzero(row)[0].tolist()) for row in used]


def used_of(sets, n_cams):
    used = np.zeros((len(sets), n_cams), bool)
    for k, s in enumerate(sets):
        used[k, sorted(s)] = True
    return used
