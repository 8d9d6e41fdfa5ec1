"""The blended full-resolution orthomosaic's CPU route (csrc/host/ortho_blend.cpp, the per-pixel rules of
csrc/ortho_blend.hpp) on the host: the reference's laplacianBlend known answers (test/test_blending.cpp) restated,
pyrDown / pyrUp against a float32 numpy restatement of the defined order, the chamfer against brute force, the colour
correction against numpy (clamps, absent cameras, the model-0 quirk), the restated exp, the float Lab round trip over all
colours, and one band of the three-camera fixture against a numpy restatement of the tile loop."""
import numpy as np
import pytest

from layers_fixtures import four_camera_scene, noise_images
from ortho_fixtures import cloud_surface, make_graph, three_cameras
from opencalibration_amd import host

A, B = 9550, 13693
INF = 0x3FFFFFFF
K = [np.float32(v) for v in (1, 4, 6, 4, 1)]


# ---- numpy restatements ---------------------------------------------------------------------------------------------

def reflect101(p, n):
    if n == 1:
        return np.zeros_like(p)
    p = np.array(p)
    while ((p < 0) | (p >= n)).any():
        p = np.where(p < 0, -p, np.where(p >= n, 2 * (n - 1) - p, p))
    return p


def _filter(img, xs, ys, scale):
    """the 5 x 5 filter in the defined order: per row k0 s0 + ... + k4 s4 left to right, then the rows top to bottom"""
    v = None
    for i in range(5):
        rows = img[ys[i]]                      # (H, w, ...)
        s = None
        for j in range(5):
            t = K[j] * rows[:, xs[j]]
            s = t if s is None else (s + t).astype(np.float32)
        t = (K[i] * s).astype(np.float32)
        v = t if v is None else (v + t).astype(np.float32)
    return (v * np.float32(scale)).astype(np.float32)


def np_pyr_down(img):
    h, w = img.shape[:2]
    H, W = (h + 1) // 2, (w + 1) // 2
    xs = [reflect101(2 * np.arange(W) + j - 2, w) for j in range(5)]
    ys = [reflect101(2 * np.arange(H) + i - 2, h) for i in range(5)]
    return _filter(img.astype(np.float32), xs, ys, 1 / 256)


def np_pyr_up(img, H, W):
    up = np.zeros((H, W) + img.shape[2:], np.float32)
    up[::2, ::2] = img[:(H + 1) // 2, :(W + 1) // 2]
    xs = [reflect101(np.arange(W) + j - 2, W) for j in range(5)]
    ys = [reflect101(np.arange(H) + i - 2, H) for i in range(5)]
    return _filter(up, xs, ys, 4 / 256)


def np_chamfer(mask):
    """brute force over every boundary pixel: b min + a (max - min) in 1e-4 units, INF with no boundary"""
    rr, cc = np.nonzero(mask)
    R, C = np.mgrid[:mask.shape[0], :mask.shape[1]]
    d = np.full(mask.shape, INF, np.int64)
    for r, c in zip(rr, cc):
        dy, dx = np.abs(R - r), np.abs(C - c)
        lo, hi = np.minimum(dx, dy), np.maximum(dx, dy)
        d = np.minimum(d, B * lo + A * (hi - lo))
    return d


def np_laplacian_blend(lab, w, levels):
    """laplacianBlend (src/ortho/blending.cpp) in float32 numpy, the defined pyramid order; returns BGR8"""
    nl, h, wd = w.shape
    f32 = np.float32
    s = np.zeros((h, wd), f32)
    for i in range(nl):
        s = (s + w[i]).astype(f32)
    s = np.maximum(s, f32(1e-6))
    nw = [(w[i] / s).astype(f32) for i in range(nl)]
    m = min(h, wd)
    lf = 1
    while (m >> lf) >= 2:
        lf += 1
    p = 1
    while p < lf and p < levels:
        p += 1
    filled = []
    for i in range(nl):
        wc, wp = [(lab[i] * nw[i][..., None]).astype(f32)], [nw[i]]
        for _ in range(1, lf):
            wc.append(np_pyr_down(wc[-1]))
            wp.append(np_pyr_down(wp[-1]))
        f = (wc[-1] / np.maximum(wp[-1], f32(1e-6))[..., None]).astype(f32)
        for l in range(lf - 2, -1, -1):
            up = np_pyr_up(f, *wp[l].shape)
            norm = (wc[l] / np.maximum(wp[l], f32(1e-6))[..., None]).astype(f32)
            f = np.where((wp[l] > f32(1e-6))[..., None], norm, up)
        filled.append(f)
    wpyr = []
    for i in range(nl):
        lv = [nw[i]]
        for _ in range(1, p):
            lv.append(np_pyr_down(lv[-1]))
        wpyr.append(lv)
    for l in range(1, p):
        ls = np.zeros_like(wpyr[0][l])
        for i in range(nl):
            ls = (ls + wpyr[i][l]).astype(f32)
        ls = np.maximum(ls, f32(1e-6))
        for i in range(nl):
            wpyr[i][l] = (wpyr[i][l] / ls).astype(f32)
    blended = []
    for l in range(p):
        acc = None
        for i in range(nl):
            g = [filled[i]]
            for _ in range(1, p):
                g.append(np_pyr_down(g[-1]))
            lap = g[l] if l == p - 1 else (g[l] - np_pyr_up(g[l + 1], *g[l].shape[:2])).astype(f32)
            t = (lap * wpyr[i][l][..., None]).astype(f32)
            acc = (np.float32(0) + t).astype(f32) if acc is None else (acc + t).astype(f32)
        blended.append(acc)
    res = blended[-1]
    for l in range(p - 2, -1, -1):
        res = (np_pyr_up(res, *blended[l].shape[:2]) + blended[l]).astype(f32)
    res = np.stack([np.clip(res[..., 0], 0, 100), np.clip(res[..., 1], -127, 127), np.clip(res[..., 2], -127, 127)], -1)
    return host.blend_math(res.reshape(-1, 3), "lab2bgr8").reshape(h, wd, 3)


# ---- laplacianBlend's known answers (test/test_blending.cpp) ----------------------------------------------------------

def flat(sz, value):
    return np.broadcast_to(np.float32(value), (sz, sz, 3)).astype(np.float32)


def test_single_layer():
    out = host.laplacian_blend(flat(64, (128, 128, 128))[None], np.ones((1, 64, 64), np.float32), 3)
    assert out.shape == (64, 64, 4) and (out[..., 3] == 255).all()
    assert (out == out[0, 0]).all()


def test_two_layers_smooth():
    sz = 64
    w = np.zeros((2, sz, sz), np.float32)
    w[0, :, :sz // 2] = 1
    w[1, :, sz // 2:] = 1
    out = host.laplacian_blend(np.stack([flat(sz, (180, 128, 128)), flat(sz, (80, 128, 128))]), w, 4)
    assert out.shape == (sz, sz, 4)
    assert out[sz // 2, sz // 4, :3].astype(int).sum() != out[sz // 2, 3 * sz // 4, :3].astype(int).sum()


def test_empty():
    assert host.laplacian_blend(np.zeros((0, 0, 0, 3)), np.zeros((0, 0, 0)), 3).size == 0


@pytest.mark.parametrize("corner", [False, True])
def test_no_ringing_at_shared_edge(corner):
    sz, nl = 128, 3
    inside = np.zeros((sz, sz), bool)
    if corner:
        inside[:3 * sz // 4, :3 * sz // 4] = True
    else:
        inside[:, :3 * sz // 4] = True
    lab = np.zeros((nl, sz, sz, 3), np.float32)
    lab[:, inside] = (50, 0, 0)
    w = np.repeat(inside[None].astype(np.float32), nl, 0)
    out = host.laplacian_blend(lab, w, 4).astype(int)
    if corner:
        ref = out[sz // 4, sz // 4, :3]
        assert np.abs(out[5:sz // 2, 5:sz // 2, :3] - ref).max() <= 2
    else:
        ref = out[sz // 2, sz // 4, :3]
        assert np.abs(out[sz // 2, :3 * sz // 4, :3] - ref).max() <= 2


def two_halves(sz, a, b):
    lab = np.zeros((sz, sz, 3), np.float32)
    lab[:, :sz // 2] = a
    lab[:, sz // 2:] = b
    return lab


def test_no_seam_at_layer_boundary():
    sz = 128
    a, b = (60, 20, 15), (40, -15, -10)
    lab = np.zeros((2, sz, sz, 3), np.float32)
    lab[0, :, :sz // 2] = a
    lab[1, :, sz // 2:] = b
    w = np.zeros((2, sz, sz), np.float32)
    w[0, :, :sz // 2] = 1
    w[1, :, sz // 2:] = 1
    out = host.laplacian_blend(lab, w, 4).astype(int)
    row = out[sz // 2]
    assert np.abs(row[5:sz // 4, :3] - row[10, :3]).max() <= 3
    assert np.abs(row[3 * sz // 4:sz - 5, :3] - row[sz - 11, :3]).max() <= 3
    for c in range(sz // 2 - 20, sz // 2 + 19):
        assert row[c, 0] >= row[c + 1, 0] - 1


def seam_weights(sz, radius):
    """the falloff of the tests' camera seam at sz / 2 through the blend's own chamfer and falloff"""
    mask = np.zeros((sz, sz), np.uint8)  # both columns beside the seam have a 4-neighbour of the other camera
    mask[:, sz // 2 - 1:sz // 2 + 1] = 1
    d = host.blend_chamfer(mask)
    df = np.where(d >= INF, np.inf, (d / 1e4)).astype(np.float32)
    steep = np.float32(np.float32(np.log(99.0)) / np.float32(radius))
    f = host.blend_math(np.stack([np.full(d.size, steep, np.float32), df.ravel()], 1), "falloff").reshape(sz, sz)
    return f


def test_boundary_only_secondary_blending():
    sz, radius = 128, 16
    a, b = (60, 10, 5), (40, -10, -5)
    lab = np.stack([two_halves(sz, a, b), two_halves(sz, b, a)])
    f = seam_weights(sz, radius)
    out = host.laplacian_blend(lab, np.stack([f, f]), 4).astype(int)
    row, margin = out[sz // 2], radius + 16
    assert np.abs(row[5:sz // 2 - margin, :3] - row[10, :3]).max() <= 2
    assert np.abs(row[sz // 2 + margin:sz - 5, :3] - row[sz - 11, :3]).max() <= 2
    for c in range(sz // 2 - radius, sz // 2 + radius - 1):
        assert row[c, 0] >= row[c + 1, 0] - 1


def test_layer_0_feathering():
    sz, radius = 128, 16
    a, b = (60, 10, 5), (40, -10, -5)
    lab = np.stack([two_halves(sz, a, b), two_halves(sz, b, a)])
    f = seam_weights(sz, radius)
    out = host.laplacian_blend(lab, np.stack([f, f]), 4).astype(int)
    assert abs(out[sz // 2, sz // 2 - 1, 0] - out[sz // 2, sz // 2, 0]) < 5


@pytest.mark.parametrize("size", [(5, 7), (37, 20), (64, 65), (70, 3)])
def test_laplacian_blend_equals_numpy(size):
    rng = np.random.default_rng(size[0])
    h, w = size
    lab = np.stack([rng.uniform(0, 100, (3, h, w)), rng.uniform(-127, 127, (3, h, w)),
                    rng.uniform(-127, 127, (3, h, w))], -1).astype(np.float32)
    wt = (rng.uniform(0, 1, (3, h, w)) * (rng.uniform(size=(3, h, w)) > 0.4)).astype(np.float32)
    got = host.laplacian_blend(lab, wt, 4)
    assert np.array_equal(got[..., :3], np_laplacian_blend(lab, wt, 4)) and (got[..., 3] == 255).all()


# ---- the defined behaviours -------------------------------------------------------------------------------------------

SIZES = list(range(1, 10)) + [37, 64, 65]


@pytest.mark.parametrize("h", SIZES)
def test_pyr_down_up_bits(h):
    rng = np.random.default_rng(h)
    for w in SIZES:
        for ch in ((), (3,)):
            img = rng.normal(0, 50, (h, w) + ch).astype(np.float32)
            down = host.blend_pyr(img)
            assert down.tobytes() == np_pyr_down(img).tobytes(), (h, w, ch)
            for H, W in {(2 * h, 2 * w), (max(1, 2 * h - 1), max(1, 2 * w - 1))}:
                assert host.blend_pyr(img, up=True, size=(H, W)).tobytes() == np_pyr_up(img, H, W).tobytes(), (h, w, H, W)


def test_chamfer_equals_brute_force():
    rng = np.random.default_rng(0)
    for trial in range(40):
        h, w = rng.integers(1, 40, 2)
        mask = (rng.uniform(size=(h, w)) < rng.choice([0.002, 0.02, 0.2])).astype(np.uint8)
        assert np.array_equal(host.blend_chamfer(mask), np_chamfer(mask)), trial
    assert (host.blend_chamfer(np.zeros((17, 9), np.uint8)) == INF).all()


def test_exp_within_one_ulp_and_falloff_limits():
    x = np.concatenate([np.linspace(0, 100, 400001), np.float32(np.log(99.0)) / 64 * np.arange(0, 6000)]).astype(np.float32)
    got = host.blend_math(x, "exp")
    with np.errstate(over="ignore"):
        ref = np.exp(x.astype(np.float64)).astype(np.float32)
    fin = np.isfinite(ref)
    ulp = np.abs(got[fin].view(np.int32).astype(np.int64) - ref[fin].view(np.int32).astype(np.int64))
    assert ulp.max() <= 1
    assert np.isinf(got[~fin]).all()
    f = host.blend_math(np.array([[0.07, 0], [0.07, np.inf], [0.07, 1e4]], np.float32), "falloff")
    assert f[0] == 1 and f[1] == 0 and f[2] == 0


def test_lab_round_trip_all_colours():
    """BGR8 -> float Lab (L1) -> BGR8 (the blend's Lab2BGR float path) over all 2^24 colours"""
    bgr = np.arange(1 << 24, dtype=np.uint32).view(np.uint8).reshape(-1, 4)[:, :3].copy()
    back = host.blend_math(host.lab_convert(bgr, "bgr2labf"), "lab2bgr8")
    diff = np.abs(back.astype(int) - bgr.astype(int)).max(1)
    # measured: every colour comes back exactly
    assert diff.max() == 0 and (diff > 0).sum() == 0


# ---- colour correction and the band -----------------------------------------------------------------------------------

def project_plain(cam, p):
    """image_from_3d with the camera record's R_inv, in float64 in the header's order"""
    d = [p[0] - cam[0], p[1] - cam[1], p[2] - cam[2]]
    R = cam[3:12]
    ray = [R[3 * i] * d[0] + R[3 * i + 1] * d[1] + R[3 * i + 2] * d[2] for i in range(3)]
    zc = 1e-3 if ray[2] < 1e-3 else ray[2]
    q = [ray[0] / zc, ray[1] / zc]
    m = cam[12:20]
    r2 = q[0] * q[0] + q[1] * q[1]
    r4 = r2 * r2
    r6 = r4 * r2
    radial = m[3] * r2 + m[4] * r4 + m[5] * r6
    prod = q[0] * q[1]
    px = [m[0] * ((1.0 + radial) * q[i] + m[6 + i] * (2.0 * prod) + m[7 - i] * (r2 + 2.0 * q[i] * q[i])) + m[1 + i]
          for i in range(2)]
    return px, ray[2]


def three_camera_band():
    pos, ori, model, _ = three_cameras()
    g = make_graph(pos, ori, model)
    pts = cloud_surface([(5, 5, -10), (10, 10, -5), (5, 10, -7.5), (10, 5, -8)])
    s = host.rebuild_mesh(np.array(pos, np.float64), previous=pts)
    plan = host.dsm_plan(g, [s], max_output_megapixels=0.02)
    imgs = noise_images(3, 600, 800, 1)
    cfg = dict(tile_size=64)
    dsm = host.dsm_render(plan, [s])
    lay = host.ortho_layers(plan, g, [s], imgs, config=cfg, dsm=dsm)
    return g, s, plan, lay, dsm, cfg


@pytest.fixture(scope="module")
def band():
    g, s, plan, lay, dsm, cfg = three_camera_band()
    yield g, s, plan, lay, dsm, cfg
    g.close()


def test_color_correction_against_numpy(band):
    g, s, plan, lay, dsm, cfg = band
    cams = host.ortho_layers_cameras(g, [s])
    ids = [int(n) for n in cams["node_ids"]]
    table = dict(per_image={ids[0]: dict(lab_offset=(-70.0, 150.0, -3.0), brdf=2.0, slope=(5.0, -4.0)),
                            ids[1]: dict(lab_offset=(1.5, -2.0, 0.5), brdf=-0.5, slope=(0.25, 3.0))},
                 per_model={0: (4.0, -2.0, 1.0), 5: (400.0, 1.0, 1.0)})
    _, plain = host.ortho_blend(plan, g, [s], lay, dsm, None, config=cfg, debug=True)
    _, got = host.ortho_blend(plan, g, [s], lay, dsm, table, config=cfg, debug=True)
    no0 = dict(table, per_model={5: (400.0, 1.0, 1.0)})
    _, got5 = host.ortho_blend(plan, g, [s], lay, dsm, no0, config=cfg, debug=True)
    valid = lay["bgra"][..., 3] > 0
    # an absent camera (ids[2]) and invalid samples: no correction
    untouched = ~valid | (lay["camera_id"] == ids[2])
    assert untouched.any() and np.array_equal(got["lab"][untouched], plain["lab"][untouched])
    f32 = np.float32
    rng = np.random.default_rng(0)
    ls, rs, cs = np.nonzero(valid & (lay["camera_id"] != ids[2]))
    pick = rng.choice(len(ls), min(400, len(ls)), replace=False)
    clamped = 0
    for k in pick:
        l, r, c = ls[k], rs[k], cs[k]
        cid = int(lay["camera_id"][l, r, c])
        ci = ids.index(cid)
        cam = cams["cams"][ci]
        p = (c * plan["gsd"] + plan["min_x"], plan["max_y"] - r * plan["gsd"], float(dsm[r, c]))
        px, rz = project_plain(cam, p)
        assert rz > 0
        t = np.array(p) - cam[:3]
        norm = np.sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2])
        cosang = cam[22] * (t[0] / norm) + cam[23] * (t[1] / norm) + cam[24] * (t[2] / norm)
        nr, nx, ny, _, va = host.ortho_sample_fields(px[0], px[1], int(cam[20]), int(cam[21]), f32(norm), cosang)
        e = table["per_image"][cid]
        lab = plain["lab"][l, r, c].copy()
        lab = (lab - np.array(e["lab_offset"], np.float32)).astype(f32)
        for vig, out in (((4.0, -2.0, 1.0), got), (None, got5)):
            L0 = lab[0]
            if vig is not None:
                r2 = f32(nr * nr)
                v = f32(f32(f32(vig[0]) * r2) + f32(f32(f32(vig[1]) * r2) * r2)) + f32(f32(f32(f32(vig[2]) * r2) * r2) * r2)
                L0 = f32(L0 - v)
            L0 = f32(L0 - f32(f32(f32(e["brdf"]) * va) * va))
            L0 = f32(L0 - f32(f32(f32(e["slope"][0]) * nx) + f32(f32(e["slope"][1]) * ny)))
            exp = np.array([np.clip(L0, 0, 100), np.clip(lab[1], -127, 127), np.clip(lab[2], -127, 127)], np.float32)
            assert exp.tobytes() == out["lab"][l, r, c].tobytes(), (l, r, c, exp, out["lab"][l, r, c])
        clamped += cid == ids[0]
    assert clamped > 0
    # the model-5 entry alone does nothing beyond the per-image terms; model 0's does
    assert not np.array_equal(got["lab"], got5["lab"])


def test_band_against_numpy_tile_loop(band):
    g, s, plan, lay, dsm, cfg = band
    T, radius = 64, 64
    rgba, dbg = host.ortho_blend(plan, g, [s], lay, dsm, None, config=cfg, debug=True)
    H, W = dsm.shape
    assert H % T and W % T  # partial last tiles
    valid = lay["bgra"][..., 3] > 0  # no sample of the fixture lies behind its camera (the layer pass skips those)
    steep = np.float32(np.float32(np.log(99.0)) / np.float32(radius))
    exp = np.zeros_like(rgba)
    for r0 in range(0, H, T):
        for c0 in range(0, W, T):
            sl = (slice(r0, r0 + T), slice(c0, c0 + T))
            v = valid[(slice(None),) + sl]
            ids0 = lay["camera_id"][(0,) + sl]
            th, tw = ids0.shape
            mask = np.zeros((th, tw), np.uint8)
            for dr, dc in ((0, -1), (0, 1), (-1, 0), (1, 0)):
                for r in range(th):
                    for c in range(tw):
                        nr_, nc_ = r + dr, c + dc
                        if v[0, r, c] and 0 <= nr_ < th and 0 <= nc_ < tw and \
                                (not v[0, nr_, nc_] or ids0[nr_, nc_] != ids0[r, c]):
                            mask[r, c] = 1
            d = np_chamfer(mask)
            df = np.where(d >= INF, np.inf, d / 1e4).astype(np.float32)
            assert df.tobytes() == dbg["dist"][sl].tobytes()
            f = host.blend_math(np.stack([np.full(df.size, steep, np.float32), df.ravel()], 1), "falloff").reshape(th, tw)
            w = dbg["weight"][(slice(None),) + sl].copy()
            w[1:] = (w[1:] * f).astype(np.float32)
            bgr = np_laplacian_blend(dbg["lab"][(slice(None),) + sl], w, 4)
            tile = np.concatenate([bgr[..., ::-1], np.full((th, tw, 1), 255, np.uint8)], -1)
            rr, cc = np.mgrid[r0:r0 + th, c0:c0 + tw]
            grey = np.where((rr + cc) % 2 == 0, 64, 128).astype(np.uint8)
            none = ~v.any(0)
            tile[none] = np.stack([grey, grey, grey, np.zeros_like(grey)], -1)[none]
            exp[sl] = tile
    assert np.array_equal(rgba, exp)
    assert (rgba[..., 3] == 0).any() and (rgba[..., 3] == 255).any()
    # the recomputed weights before the falloff are the layer pass's
    assert np.array_equal(dbg["weight"].view(np.uint32), lay["weight"].view(np.uint32))


def test_mosaic_bands_equal_one_call():
    g, s, imgs = four_camera_scene(seed=5)
    plan = dict(width=70, height=140, gsd=0.1, min_x=-1.0, max_x=6.0, min_y=-2.0, max_y=12.0, mean_camera_z=10.0)
    cfg = dict(tile_size=32)
    whole = host.ortho_mosaic(plan, g, [s], imgs, config=cfg, tile_rows=5)
    bands = host.ortho_mosaic(plan, g, [s], imgs, config=cfg, tile_rows=1)
    assert np.array_equal(whole, bands) and whole.shape == (140, 70, 4)
    g.close()
