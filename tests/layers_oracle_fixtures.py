"""A long-double reference of the layered orthomosaic's per-pixel rules (csrc/ortho_layers.hpp), written from the rules
and not from the header's expressions: true pow / cbrt / arccos, a hand-differentiated Jacobian and no jets, whole
rasters at a time in numpy.  No import of the library.

Every comparison that decides something (a branch, a truncation, a rounding) also says whether its operand lies within
EDGE of the edge; a pixel with any such flag is ambiguous: there the reference and a double implementation may
legitimately part, so the tests leave it out and count it."""
import numpy as np

LD = np.longdouble if np.finfo(np.longdouble).nmant > 52 else np.float64
EDGE = LD("1e-9")
NONE = 0xFFFFFFFF
f32 = np.float32


def ld(v):
    return np.asarray(v, dtype=LD)


def near(v, edge):
    """v within EDGE of the edge, relative to the larger of 1 and the edge's magnitude"""
    edge = ld(edge)
    return np.abs(v - edge) <= EDGE * np.maximum(LD(1), np.abs(edge))


def f32_tie_near(v, of_value=False):
    """v within EDGE of a value half way between two neighbouring float32: relative to the float32 spacing there, or
    (of_value) to the value itself.  The second band holds 2e-9 / 2^-23, some 2 %, of all values: it serves where a
    value on it is still compared (to one ulp), the first where a pixel on it is left out."""
    v = ld(v)
    f = v.astype(f32)
    up, dn = ld(np.nextafter(f, f32(np.inf))), ld(np.nextafter(f, f32(-np.inf)))
    d = np.minimum(np.abs(v - (ld(f) + up) / 2), np.abs(v - (ld(f) + dn) / 2))
    return d <= EDGE * (np.abs(v) if of_value else (up - dn) / 2)


# ---- colour: OpenCV's documented BGR <-> L*a*b* (sRGB curve, D65) -------------------------------------------------------
RGB2XYZ = ld([[LD(s) for s in r] for r in (("0.412453", "0.357580", "0.180423"), ("0.212671", "0.715160", "0.072169"),
                                            ("0.019334", "0.119193", "0.950227"))])
XYZ2RGB = ld([[LD(s) for s in r] for r in (("3.240479", "-1.53715", "-0.498535"), ("-0.969256", "1.875991", "0.041556"),
                                            ("0.055648", "-0.204043", "1.057311"))])
XN, ZN = LD("0.950456"), LD("1.088754")
T0, K7, K903 = LD("0.008856"), LD("7.787"), LD("903.3")
OFF = LD(16) / LD(116)


def srgb_decode(c):
    c = ld(c)
    return np.where(c <= LD("0.04045"), c / LD("12.92"), ((c + LD("0.055")) / LD("1.055")) ** LD("2.4"))


LIN = srgb_decode(np.arange(256, dtype=LD) / 255)                      # linear value of code v
THR = srgb_decode((np.arange(255, dtype=LD) + LD("0.5")) / 255)        # linear value half a code above code k


def bgr2lab(bgr):
    """(..., 3) uint8 BGR -> (..., 3) L*a*b*, L in 0..100, unrounded"""
    lin = LIN[np.asarray(bgr, np.uint8)]
    # every row of the matrix sums to its white, so X / Xn, Y and Z / Zn are G plus multiples of R - G and B - G: taken
    # that way a grey's a and b are 0 here as they are in exact arithmetic, not this module's own rounding (2.7e-17)
    assert RGB2XYZ.sum(1).astype(np.float64).tolist() == [float(XN), 1.0, float(ZN)]
    G, dR, dB = lin[..., 1], lin[..., 2] - lin[..., 1], lin[..., 0] - lin[..., 1]
    X = G + (RGB2XYZ[0, 0] * dR + RGB2XYZ[0, 2] * dB) / XN
    Y = G + RGB2XYZ[1, 0] * dR + RGB2XYZ[1, 2] * dB
    Z = G + (RGB2XYZ[2, 0] * dR + RGB2XYZ[2, 2] * dB) / ZN
    f = lambda t: np.where(t > T0, np.cbrt(t), K7 * t + OFF)
    fx, fy, fz = f(X), f(Y), f(Z)
    L = np.where(Y > T0, 116 * fy - 16, K903 * Y)
    return np.stack([L, 500 * (fx - fy), 200 * (fy - fz)], -1)


def bgr2lab8(bgr):
    """8-bit Lab (L * 255 / 100, a + 128, b + 128, to nearest, saturated) and per colour the margin: the smallest
    distance of a channel's unrounded value from a rounding tie (k + 0.5)"""
    lab = bgr2lab(bgr)
    v = np.stack([lab[..., 0] * 255 / 100, lab[..., 1] + 128, lab[..., 2] + 128], -1)
    code = np.clip(np.floor(v + LD("0.5")), 0, 255).astype(np.uint8)
    margin = np.abs(v - np.floor(v) - LD("0.5")).min(-1)
    return code, margin


def bgr2labf(bgr):
    """float32 Lab and, per channel, whether the unrounded value is within EDGE (of its size) of a float32 tie"""
    lab = bgr2lab(bgr)
    return lab.astype(f32), f32_tie_near(lab, of_value=True)


def lab82bgr(lab8):
    """8-bit Lab -> BGR codes; the code of a linear value is the number of half-code thresholds at or below it.  The
    margin is the smallest distance, in codes, of a channel's encoded value from a tie (k + 0.5)."""
    lab8 = ld(np.asarray(lab8, np.uint8))
    L, a, b = lab8[..., 0] * 100 / 255, lab8[..., 1] - 128, lab8[..., 2] - 128
    low = L <= 8
    Y = np.where(low, L / K903, ((L + 16) / 116) ** 3)
    fy = np.where(low, K7 * (L / K903) + OFF, (L + 16) / 116)
    f_inv = lambda f: np.where(f > LD("0.206893"), f ** 3, (f - OFF) / K7)
    xyz = np.stack([f_inv(fy + a / 500) * XN, Y, f_inv(fy - b / 200) * ZN], -1)
    rgb = np.stack([(xyz * XYZ2RGB[i]).sum(-1) for i in range(3)], -1)
    lin = rgb[..., ::-1]
    code = np.searchsorted(THR, lin.ravel(), side="right").reshape(lin.shape)
    c = np.clip(lin, 0, 1)  # below code 0 or above code 255: as far from a tie as those codes themselves
    c = 255 * np.where(c <= LD("0.04045") / LD("12.92"), c * LD("12.92"), LD("1.055") * c ** (1 / LD("2.4")) - LD("0.055"))
    return code.astype(np.uint8), np.abs(c - np.floor(c) - LD("0.5")).min(-1)


# ---- projection ------------------------------------------------------------------------------------------------------------
class Cameras:
    """positions (n, 3), orientations (n, 4; x y z w, camera to world), models (n, 10): f ppx ppy k1 k2 k3 p1 p2 cols rows"""

    def __init__(self, positions, orientations, models10):
        self.pos = ld(positions).reshape(-1, 3)
        q = ld(orientations).reshape(-1, 4)
        x, y, z, w = (q / np.sqrt((q * q).sum(1))[:, None]).T
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=LD)  # [i][j][n]
        self.R_inv = np.transpose(R, (2, 1, 0))  # [n][j][i]: the transpose of each rotation
        self.model = ld(np.broadcast_to(np.asarray(models10, np.float64), (len(self.pos), 10)))
        self.cols = self.model[:, 8].astype(np.int64)
        self.rows = self.model[:, 9].astype(np.int64)


def project(C, ci, x, y, z, jacobian=True):
    """camera ci[k] at world point k: z of R_inv (p - position), the pixel (P, 2) and d pixel / d (x, y) (P, 2, 2)"""
    ci = np.asarray(ci, np.int64)
    p = np.stack([ld(x), ld(y), ld(z)], -1)
    Ri = C.R_inv[ci]
    ray = np.einsum("kij,kj->ki", Ri, p - C.pos[ci])
    clamped = ray[:, 2] < LD("1e-3")
    zc = np.where(clamped, LD("1e-3"), ray[:, 2])
    u, v = ray[:, 0] / zc, ray[:, 1] / zc
    f, ppx, ppy, k1, k2, k3, t1, t2 = (C.model[ci, i] for i in range(8))
    r2 = u * u + v * v
    g = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    du = u * g + 2 * t1 * u * v + t2 * (r2 + 2 * u * u)
    dv = v * g + 2 * t2 * u * v + t1 * (r2 + 2 * v * v)
    pixel = np.stack([f * du + ppx, f * dv + ppy], -1)
    if not jacobian:
        return ray[:, 2], pixel
    gp = k1 + 2 * k2 * r2 + 3 * k3 * r2 ** 2  # d g / d r2
    D = np.empty((len(ci), 2, 2), LD)         # d (du, dv) / d (u, v)
    D[:, 0, 0] = g + 2 * u * u * gp + 2 * t1 * v + 6 * t2 * u
    D[:, 0, 1] = 2 * u * v * gp + 2 * t1 * u + 2 * t2 * v
    D[:, 1, 0] = 2 * u * v * gp + 2 * t2 * v + 2 * t1 * u
    D[:, 1, 1] = g + 2 * v * v * gp + 2 * t2 * u + 6 * t1 * v
    # d (u, v) / d (x, y): the ray moves by R_inv's first two columns; a clamped z is a constant
    dz = np.where(clamped[:, None], LD(0), Ri[:, 2, :2])
    Pm = np.stack([(Ri[:, 0, :2] - u[:, None] * dz) / zc[:, None], (Ri[:, 1, :2] - v[:, None] * dz) / zc[:, None]], 1)
    return ray[:, 2], pixel, f[:, None, None] * np.einsum("kij,kjl->kil", D, Pm)


# ---- the ellipse sampler ---------------------------------------------------------------------------------------------------
MAX_RADIUS = 16


class Image:
    """a source image with its reference 8-bit Lab and where that conversion sits on a rounding tie"""

    def __init__(self, bgr):
        self.bgr = np.asarray(bgr, np.uint8)
        lab8, margin = bgr2lab8(self.bgr)
        self.lab8 = lab8.astype(np.int64)
        self.tie = margin < EDGE


def sample(image, pixel, J, gsd):
    """The colour of the output pixel whose gsd x gsd square maps to the ellipse M = gsd^2 J J^T around `pixel` (P, 2; inside
    the image; gsd a scalar or one per point): the pixel under it when the ellipse is smaller than a pixel or degenerate, else the truncated mean 8-bit
    Lab of the pixel centres inside it, back in BGR.  Returns bgr (P, 3), ambiguous (P) and the branch facts."""
    rows, cols = image.bgr.shape[:2]
    pixel, J = ld(pixel).reshape(-1, 2), ld(J).reshape(-1, 2, 2)
    M = (ld(gsd) ** 2).reshape(-1, 1, 1) * np.einsum("kij,klj->kil", J, J)
    m00, m01, m11 = M[:, 0, 0], M[:, 0, 1], M[:, 1, 1]
    half, disc = (m00 + m11) / 2, np.sqrt(((m00 - m11) / 2) ** 2 + m01 ** 2)
    a = np.sqrt(np.maximum(half + disc, LD("1e-6")))
    b = np.sqrt(np.maximum(half - disc, LD("1e-6")))
    det = m00 * m11 - m01 * m01
    amb = near(a, 1) | near(b, 1) | near(det, LD("1e-12")) | near(pixel, np.rint(pixel)).any(-1)
    ix, iy = np.floor(pixel[:, 0]).astype(np.int64), np.floor(pixel[:, 1]).astype(np.int64)
    out = image.bgr[iy, ix].copy()
    single = ((a < 1) & (b < 1)) | (det < LD("1e-12"))
    ell = np.nonzero(~single)[0]
    radius = np.zeros(len(pixel), np.int64)
    count = np.zeros(len(pixel), np.int64)
    if len(ell):
        amb[ell] |= near(a[ell], np.rint(a[ell]))
        radius[ell] = np.minimum(np.ceil(a[ell]), MAX_RADIUS).astype(np.int64)
        i00, i01, i11 = m11[ell] / det[ell], -m01[ell] / det[ell], m00[ell] / det[ell]
        total = np.zeros((len(ell), 3), np.int64)
        n, touched = np.zeros(len(ell), np.int64), np.zeros(len(ell), bool)
        rad, ex, ey = radius[ell], ix[ell], iy[ell]
        for oy in range(-rad.max(), rad.max() + 1):
            for ox in range(-rad.max(), rad.max() + 1):
                px, py = ex + ox, ey + oy
                k = np.nonzero((abs(ox) <= rad) & (abs(oy) <= rad) & (px >= 0) & (px < cols) & (py >= 0) & (py < rows))[0]
                dx, dy = px[k] - pixel[ell[k], 0], py[k] - pixel[ell[k], 1]
                e = i00[k] * dx * dx + 2 * i01[k] * dx * dy + i11[k] * dy * dy
                touched[k] |= np.abs(e - 1) <= EDGE
                k, inside = k[e <= 1], (px[k][e <= 1], py[k][e <= 1])
                total[k] += image.lab8[inside[1], inside[0]]
                touched[k] |= image.tie[inside[1], inside[0]]
                n[k] += 1
        amb[ell] |= touched
        count[ell] = n
        has = n > 0
        back, margin = lab82bgr((total[has] // n[has, None]).astype(np.uint8))
        out[ell[has]] = back
        amb[ell[has]] |= margin < EDGE
    return out, amb, dict(a=a, b=b, single=single, radius=radius, count=count)


# ---- the sample's fields ---------------------------------------------------------------------------------------------------
def blend_weight_f32(px, py, width, height, distance):
    """computeBlendWeight step by step in float32: the distance to the nearest image edge over half the width (0.001 ..
    1), times 1 - half the normalised distance from the centre (at most 1), times 1 / (1 + distance^2).  px, py,
    distance: float32."""
    px, py, d = np.asarray(px, f32), np.asarray(py, f32), np.asarray(distance, f32)
    w, h = np.asarray(width).astype(f32), np.asarray(height).astype(f32)
    hw, hh = w * f32(0.5), h * f32(0.5)
    edge = np.minimum(np.minimum(px, w - f32(1) - px), np.minimum(py, h - f32(1) - py))
    ew = np.maximum(np.minimum((edge / hw).astype(f32), f32(1)), f32(0.001))
    cx, cy = ((px - hw) / hw).astype(f32), ((py - hh) / hh).astype(f32)
    cw = f32(1) - f32(0.5) * np.minimum(np.sqrt((cx * cx + cy * cy).astype(f32)), f32(1))
    prox = f32(1) / (f32(1) + d * d)
    return ((ew * cw).astype(f32) * prox).astype(f32)


def fields(C, ci, pixel, x, y, z):
    """normalised radius, x, y and the view angle as the correctly rounded float32 of their long-double values, the
    blend weight by its float32 restatement on float32(pixel) and float32(distance); and where those two roundings sit
    on a float32 tie"""
    ci = np.asarray(ci, np.int64)
    hw, hh = ld(C.cols[ci]) / 2, ld(C.rows[ci]) / 2
    nx, ny = (pixel[:, 0] - hw) / hw, (pixel[:, 1] - hh) / hh
    radius = np.clip(np.sqrt(nx * nx + ny * ny) / np.sqrt(LD(2)), 0, 1)
    t = np.stack([ld(x), ld(y), ld(z)], -1) - C.pos[ci]
    dist = np.sqrt((t * t).sum(-1))
    down = C.R_inv[ci][:, :, 2]  # orientation^-1 (0, 0, 1)
    angle = np.arccos(np.clip((down * t).sum(-1) / dist, -1, 1))
    four = np.stack([radius, np.clip(nx, -1, 1), np.clip(ny, -1, 1), angle], -1).astype(f32)
    weight = blend_weight_f32(pixel[:, 0].astype(f32), pixel[:, 1].astype(f32), C.cols[ci], C.rows[ci], dist.astype(f32))
    return four, weight, f32_tie_near(pixel).any(-1) | f32_tie_near(dist)


# ---- one band's layers -----------------------------------------------------------------------------------------------------
def render(plan, C, images, node_ids, knn, dsm, num_layers, row0=0):
    """Per pixel: walk its kNN list (camera indices, NONE-padded), skip a camera behind whose image plane the point lies
    (ray z <= 0) or whose pixel falls outside [0, cols) x [0, rows), fill up to num_layers layers; the rest are invalid
    samples (all zero).  A NaN height leaves every layer invalid.  images: a list of Image.  Returns the planes bgra,
    camera (index, -1 invalid), camera_id, weight, fields (L, rows, width, ...), ambiguous (rows, width) and counts of
    the branches taken."""
    rows, width = dsm.shape
    N, L = rows * width, num_layers
    gsd = LD(plan["gsd"])
    x = ld(np.tile(np.arange(width), rows)) * gsd + LD(plan["min_x"])
    y = LD(plan["max_y"]) - ld(np.repeat(np.arange(row0, row0 + rows), width)) * gsd
    z = ld(np.asarray(dsm, f32).ravel())
    open_ = ~np.isnan(z)
    knn = np.asarray(knn).reshape(N, -1)
    n = np.zeros(N, np.int64)
    bgra, camera = np.zeros((L, N, 4), np.uint8), np.full((L, N), -1, np.int64)
    weight, four = np.zeros((L, N), f32), np.zeros((L, N, 4), f32)
    amb = np.zeros(N, bool)
    stats = dict(nan=int((~open_).sum()), behind=0, outside=0, single=0, ellipse=0, a_over_1_over_b=0, capped=0, empty=0,
                 clipped=0, max_radius=0)
    for k in range(knn.shape[1]):
        open_ &= knn[:, k] != NONE
        idx = np.nonzero(open_ & (n < L))[0]
        if not len(idx):
            continue
        ci = knn[idx, k].astype(np.int64)
        rz, pixel, J = project(C, ci, x[idx], y[idx], z[idx])
        amb[idx] |= near(rz, 0) | near(rz, LD("1e-3"))
        front = rz > 0
        cols, rws = ld(C.cols[ci]), ld(C.rows[ci])
        px, py = pixel[:, 0], pixel[:, 1]
        amb[idx] |= front & (near(px, 0) | near(px, cols) | near(py, 0) | near(py, rws))
        inside = (px >= 0) & (px < cols) & (py >= 0) & (py < rws)
        stats["behind"] += int((~front).sum())
        stats["outside"] += int((front & ~inside).sum())
        ok = front & inside
        j, cj, pixel, J = idx[ok], ci[ok], pixel[ok], J[ok]
        bgr, flag = np.zeros((len(j), 3), np.uint8), np.zeros(len(j), bool)
        for c in np.unique(cj):
            s = cj == c
            bgr[s], flag[s], info = sample(images[c], pixel[s], J[s], gsd)
            ell = ~info["single"]
            r = info["radius"][ell]
            stats["single"] += int(info["single"].sum())
            stats["ellipse"] += int(ell.sum())
            stats["a_over_1_over_b"] += int(((info["a"] > 1) & (info["b"] < 1)).sum())
            stats["capped"] += int((info["a"][ell] > MAX_RADIUS).sum())
            stats["empty"] += int((info["count"][ell] == 0).sum())
            stats["max_radius"] = max(stats["max_radius"], int(r.max()) if len(r) else 0)
            fx, fy = np.floor(pixel[s][ell, 0]), np.floor(pixel[s][ell, 1])
            stats["clipped"] += int(((fx - r < 0) | (fy - r < 0) | (fx + r > C.cols[c] - 1) | (fy + r > C.rows[c] - 1)).sum())
        fo, w, tie = fields(C, cj, pixel, x[j], y[j], z[j])
        amb[j] |= flag | tie
        layer = n[j]
        bgra[layer, j, :3], bgra[layer, j, 3] = bgr, 255
        camera[layer, j], weight[layer, j], four[layer, j] = cj, w, fo
        n[j] += 1
    ids = np.asarray(node_ids, np.uint64)
    camera_id = np.where(camera >= 0, ids[np.maximum(camera, 0)], np.uint64(0)).astype(np.uint64)
    shape = (L, rows, width)
    return dict(bgra=bgra.reshape(shape + (4,)), camera=camera.reshape(shape), camera_id=camera_id.reshape(shape),
                weight=weight.reshape(shape), fields=four.reshape(shape + (4,)), ambiguous=amb.reshape(rows, width),
                stats=stats)


# ---- the colour correspondences of a finished band -------------------------------------------------------------------------
def sampled_pixels(camera_id, valid, tile, subsample):
    """Which pixels emit records: inside its tile a pixel is a boundary pixel when a valid 4-neighbour holds another
    layer-0 camera; boundary pixels are taken where (local row + local col) % subsample == 0, the others where both are
    multiples; only pixels with a valid layer 0.  In the canonical order: tiles row-major, then local raster order."""
    rows, cols = camera_id.shape[1:]
    out = []
    for r0 in range(0, rows, tile):
        for c0 in range(0, cols, tile):
            for r in range(r0, min(r0 + tile, rows)):
                for c in range(c0, min(c0 + tile, cols)):
                    if not valid[0, r, c]:
                        continue
                    boundary = False
                    for nr, nc in ((r, c - 1), (r, c + 1), (r - 1, c), (r + 1, c)):
                        if r0 <= nr < min(r0 + tile, rows) and c0 <= nc < min(c0 + tile, cols):
                            boundary |= bool(valid[0, nr, nc]) and camera_id[0, nr, nc] != camera_id[0, r, c]
                    lr, lc = r - r0, c - c0
                    if (lr + lc) % subsample == 0 if boundary else lr % subsample == 0 and lc % subsample == 0:
                        out.append((r, c))
    return out


def correspondences(bgra, camera_id, tile, radius, subsample):
    """The records of a finished band (the route's own bgra (L, rows, cols, 4) and camera_id planes): per sampled pixel
    and pair of valid layers a < b, the mean Lab of each layer over the window |dr|, |dc| <= radius clipped at the
    tile, counting a pixel only where layer b is valid and both layers hold the centre's cameras.  Returns a list of
    dict(row, col, layer_a, layer_b, count, mean_a, mean_b (long double, of the unrounded Lab), abs_a, abs_b (sum |lab|))."""
    valid = bgra[..., 3] == 255
    lab = bgr2lab(bgra[..., :3])
    rows, cols = camera_id.shape[1:]
    out = []
    if subsample <= 0:
        return out
    for r, c in sampled_pixels(camera_id, valid, tile, subsample):
        r0, c0 = r // tile * tile, c // tile * tile
        rs = slice(max(r - radius, r0), min(r + radius, r0 + tile - 1, rows - 1) + 1)
        cs = slice(max(c - radius, c0), min(c + radius, c0 + tile - 1, cols - 1) + 1)
        n = int(valid[:, r, c].sum())
        for a in range(n):
            for b in range(a + 1, n):
                m = valid[b, rs, cs] & (camera_id[a, rs, cs] == camera_id[a, r, c]) & (camera_id[b, rs, cs] == camera_id[b, r, c])
                la, lb = lab[a, rs, cs][m], lab[b, rs, cs][m]
                k = int(m.sum())
                out.append(dict(row=r, col=c, layer_a=a, layer_b=b, count=k, mean_a=la.sum(0) / k, mean_b=lb.sum(0) / k,
                                abs_a=np.abs(la).sum(0), abs_b=np.abs(lb).sum(0)))
    return out


def mean_bound(count, abs_sum):
    """|float32 mean - exact mean| per channel: recursive float summation of count terms (count - 1 roundings), one
    rounding of each input to float and two for the reciprocal scaling"""
    return (count + 2) * LD(2) ** -24 * abs_sum / count
