"""An fp64 model of AKAZE's nonlinear scale space for test_akaze_planes_oracle.py (the restatement oracle/akaze.cpp against
it) and test_gpu_akaze_planes.py (the device against both), with the images, the tolerance table and the helper that says
where two planes differ.

The model is plain numpy float64, vectorised and written from the definitions (the functions' docstrings state them), not from
the restatement's loops: whole-plane slices, padded borders, overlap matrices for the resize.  It shares no code and no table
with oracle/ or csrc/akaze.hip.  `mutation` introduces ONE deliberate error (MUTATIONS); the CPU tests require each of them to
miss the tolerance table by a factor of 100 somewhere, which is what keeps the table honest.

THE TOLERANCES.  TOLERANCE[plane][level] is 4 x MEASURED[plane][level], the largest |oracle - model| over every pixel of the
level over the images of IMAGES (the restatement built with g++ -O3 -ffp-contract=off on x86-64; the test prints the observed
figures under -s, and measure_oracle_errors() below regenerates the table).  The measured figure is already the extreme of
1e4 - 2e5 pixels and the images stay within a factor of 2 of each other; 4 x leaves room for another compiler's libm in the
Gaussian taps without masking a real deviation: the mutations move the planes by 6e4 - 5e5 times the tolerance.
In short: Lt 2.4e-7 - 3.4e-7 at levels 0 - 11 (values up to 1), Lx / Ly 2e-8 - 5.4e-8, Ldet 2e-9 - 3.2e-8.

THE COARSE LEVELS.  The last octave of the 640 x 320 images (80 x 40, FED cycles of 17 - 29 steps) is further from fp64 on Lt
than the other levels: 6.1e-7 at level 12 and 8.5e-7 at level 15 against 3e-7 elsewhere.  That is the restatement's fp32
round-off amplified by the cycle's super-stable steps (its largest step is ~ 0.2 n^2 times the explicit limit); those levels
have their own entries.  It is a factor of 3, NOT the 6e-5 a model shows that takes the steps of a cycle in ascending order:
that figure is the fp64 MODEL's own instability - in ascending order fp64 itself is 4.9e-5 away from long double at level 15
(3.2e-7 at level 14, 5e-9 at level 13) -, which is why fed_steps orders a cycle by Leja's rule.  With it the model is within
5e-16 of its long-double evaluation at every level (test_the_model_against_long_double holds it there).
"""
import functools
import math

import numpy as np

from opencalibration_amd import synth

PLANES = ("Lt", "Lx", "Ly", "Ldet")

# name -> (width, height, seed of synth.render_blobs, amplitude of the uniform pixel noise)
IMAGES = {
    "blobs_640x320": (640, 320, 31, 0),     # four octaves down to 80 x 40, the smallest octave allowed; every side halves exactly
    "noisy_640x320": (640, 320, 31, 40),
    "noisy_501x334": (501, 334, 31, 40),    # odd sides: the general area path between the octaves, three octaves
    "noisy_176x96": (176, 96, 31, 40),      # two octaves: the smallest case with an octave change
}
EXACT_HALVING = ("blobs_640x320", "noisy_640x320", "noisy_176x96")

MUTATIONS = (
    "sobel_conductivity",          # (1, 2, 1) instead of (3, 10, 3) in the conductivity's gradient
    "no_octave_factor",            # the contrast factor is not multiplied by 0.75 at a new octave
    "reflecting_diffusion_border",  # the diffusion step sees a reflected neighbour beyond the border instead of no flux
    "derivatives_on_lt",           # Lx, Ly, Ldet from the level's Lt instead of its Lsmooth
    "det_s2",                      # Ldet scaled by s^2 instead of s^4
    "decimation",                  # a new octave takes every second pixel instead of the 2 x 2 mean
)


@functools.lru_cache(maxsize=None)
def image(name):
    """the grey 8-bit image of a case (h x w); its BGR form for the device is bgr(name)"""
    w, h, seed, amp = IMAGES[name]
    base = synth.render_blobs(w, h, seed, channels=1)
    if amp:
        rng = np.random.default_rng(w)
        base = np.clip(base.astype(np.int32) + rng.integers(0, amp, (h, w)) - amp // 2, 0, 255).astype(np.uint8)
    base.setflags(write=False)
    return base


def bgr(name_or_grey):
    g = image(name_or_grey) if isinstance(name_or_grey, str) else name_or_grey
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))


def constant_image(w=176, h=96, value=127):
    return np.full((h, w), value, np.uint8)


def ramp_image(w=256, h=96):
    """grey value = column: the steepest exactly linear 8-bit image (slope 1 / 255 per pixel), two octaves"""
    return np.ascontiguousarray(np.broadcast_to(np.arange(w, dtype=np.uint8)[None, :], (h, w)))


# ------------------------------------------------------------------------------------------------------------ the model
def level_table(w, h):
    """Up to 4 octaves x 4 sublevels; octave o is (w >> o) x (h >> o) and the table ends with the first octave below 80 wide or 40
    high; sigma = 1.6 * 2^(o + j / 4), derivative scale s = lrint(float32(sigma) * 1.5 / 2^o), evolution time t = sigma^2 / 2."""
    levels = []
    for o in range(4):
        lw, lh = w >> o, h >> o
        if o and (lw < 80 or lh < 40):
            break
        for j in range(4):
            sigma = 1.6 * 2.0 ** (o + j / 4.0)
            s = int(np.rint(np.float32(sigma) * np.float32(1.5) / np.float32(1 << o)))
            levels.append({"octave": o, "sublevel": j, "width": lw, "height": lh, "sigma": sigma, "sigma_size": s, "etime": 0.5 * sigma * sigma})
    return levels


def gaussian_taps(sigma):
    """cv::GaussianBlur's sizing ceil(2 (1 + (sigma - 0.8) / 0.3)) made odd, exp(-x^2 / (2 sigma^2)) normalised to sum 1"""
    n = int(math.ceil(2.0 * (1.0 + (sigma - 0.8) / 0.3)))
    n += 1 - n % 2
    x = np.arange(n) - n // 2
    k = np.exp(-0.5 * x * x / (sigma * sigma))
    return k / k.sum()


def gaussian(img, sigma):
    """separable, replicated border"""
    k = gaussian_taps(sigma)
    r = len(k) // 2
    h, w = img.shape
    p = np.pad(img, ((0, 0), (r, r)), mode="edge")
    rows = sum(k[t] * p[:, t:t + w] for t in range(len(k)))
    p = np.pad(rows, ((r, r), (0, 0)), mode="edge")
    return sum(k[t] * p[t:t + h, :] for t in range(len(k)))


def scharr(img, s, side, centre):
    """(d/dx, d/dy) by the 3 x 3 pattern spread to distance s: the central difference over 2 s weighted side : centre : side across
    it, reflect-101 border, unnormalised"""
    h, w = img.shape
    p = np.pad(img, s, mode="reflect")
    dx = p[:, 2 * s:] - p[:, :w]                       # I(x + s) - I(x - s), every padded row
    dy = p[2 * s:, :] - p[:h, :]
    gx = side * dx[:h] + centre * dx[s:s + h] + side * dx[2 * s:]
    gy = side * dy[:, :w] + centre * dy[:, s:s + w] + side * dy[:, 2 * s:]
    return gx, gy


def contrast_factor(img):
    """Gaussian(1) of the input, unnormalised Scharr (3, 10, 3), gradient magnitude on the interior pixels, 300 bins with bin
    int(m * 299 / hmax) - bin 0 is the background -; the factor is hmax * k / 300 at the first k >= 1 whose bins 1 .. k - 1 hold
    int((interior - hist[0]) * 0.7f) pixels (a float32 product: it decides an integer); a blank image gives 0.03.
    Returns (factor, k, hmax)."""
    gx, gy = scharr(gaussian(img, 1.0), 1, 3.0, 10.0)
    m = np.sqrt(gx * gx + gy * gy)[1:-1, 1:-1]
    hmax = m.max()
    if hmax == 0.0:
        return 0.03, 0, 0.0
    hist = np.bincount((m * (299.0 / hmax)).astype(np.int64).ravel(), minlength=300)
    need = int(np.float32(m.size - hist[0]) * np.float32(0.7))
    below = np.concatenate([[0], np.cumsum(hist[1:])])     # below[k - 1]: pixels in bins 1 .. k - 1
    for k in range(1, 300):
        if below[k - 1] >= need:
            return hmax * k / 300.0, k, hmax
    return 0.03, 0, hmax


def fed_steps(T):
    """tau_j = 0.25 / (2 cos^2(pi (2 j + 1) / (4 n + 2))) scaled by 3 T / (0.25 n (n + 1)), n = ceil(sqrt(3 T / 0.25 + 0.25) - 0.5 - 1e-8).
    The steps of a cycle commute (the conductivity is fixed); they are taken in the order that keeps fp64's round-off smallest:
    by Leja's rule on 1 / tau, each next step the one furthest (in product) from those taken."""
    n = int(math.ceil(math.sqrt(3.0 * T / 0.25 + 0.25) - 0.5 - 1e-8))
    j = np.arange(n)
    tau = 0.25 / (2.0 * np.cos(math.pi * (2 * j + 1) / (4 * n + 2)) ** 2) * (3.0 * T / (0.25 * n * (n + 1)))
    nodes, order, left = 1.0 / tau, [], list(range(n))
    while left:
        score = [nodes[i] if not order else np.sum(np.log(np.abs(nodes[i] - nodes[order]))) for i in left]
        order.append(left.pop(int(np.argmax(score))))
    return tau[order]


def diffusion_step(L, c, tau, mutation=None):
    """L += tau / 2 * sum over the four faces of (c_a + c_b) (L_b - L_a), no flux through the image border"""
    if mutation == "reflecting_diffusion_border":
        Lp, cp = np.pad(L, 1, mode="reflect"), np.pad(c, 1, mode="reflect")
        mid, cm = Lp[1:-1, 1:-1], cp[1:-1, 1:-1]
        div = sum((cm + cp[sl]) * (Lp[sl] - mid) for sl in ((slice(1, -1), slice(2, None)), (slice(1, -1), slice(None, -2)),
                                                          (slice(2, None), slice(1, -1)), (slice(None, -2), slice(1, -1))))
        return L + 0.5 * tau * div
    fx = (c[:, 1:] + c[:, :-1]) * (L[:, 1:] - L[:, :-1])
    fy = (c[1:, :] + c[:-1, :]) * (L[1:, :] - L[:-1, :])
    div = np.zeros_like(L)
    div[:, :-1] += fx
    div[:, 1:] -= fx
    div[:-1, :] += fy
    div[1:, :] -= fy
    return L + 0.5 * tau * div


def _overlap_matrix(n_src, n_dst):
    """row d: the shares of the source pixels in [d scale, (d + 1) scale) cut at the image's end, scale = n_src / n_dst"""
    scale = n_src / n_dst
    lo = np.arange(n_dst)[:, None] * scale
    hi = np.minimum(lo + scale, n_src)
    px = np.arange(n_src)[None, :]
    share = np.clip(np.minimum(hi, px + 1.0) - np.maximum(lo, px), 0.0, None)
    return share / (hi - lo)


def half_sample(L, w, h, mutation=None):
    """to w x h: the 2 x 2 mean when both sides halve exactly, else the area-weighted mean over the exact footprint on both axes"""
    sh, sw = L.shape
    if mutation == "decimation":
        return L[(np.arange(h) * sh) // h][:, (np.arange(w) * sw) // w].copy()
    if sw == 2 * w and sh == 2 * h:
        return 0.25 * (L[0::2, 0::2] + L[0::2, 1::2] + L[1::2, 0::2] + L[1::2, 1::2])
    return _overlap_matrix(sh, h) @ L @ _overlap_matrix(sw, w).T


def scale_space(grey, kcontrast=None, mutation=None, dtype=np.float64):
    """The scale space of an 8-bit grey image (values / 255): {"kcontrast", "k_bin", "hmax", "levels": [level_table's rows + the
    float64 planes Lt, Lsmooth, Lx, Ly, Ldet]}.  kcontrast: the contrast factor from outside instead of the model's own.
    dtype=np.longdouble: the planes in the platform's long double (the tables stay float64), which measures the model's own
    round-off."""
    assert mutation is None or mutation in MUTATIONS, mutation
    img = np.asarray(grey, dtype) / 255.0
    h, w = img.shape
    levels = level_table(w, h)
    own_k, k_bin, hmax = contrast_factor(img)
    k = float(own_k if kcontrast is None else kcontrast)
    side, centre = (1.0, 2.0) if mutation == "sobel_conductivity" else (3.0, 10.0)
    levels[0]["Lt"] = levels[0]["Lsmooth"] = gaussian(img, 1.6)
    for i in range(1, len(levels)):
        l, p = levels[i], levels[i - 1]
        L = p["Lt"]
        if l["octave"] > p["octave"]:
            L = half_sample(L, l["width"], l["height"], mutation)
            if mutation != "no_octave_factor":
                k *= 0.75
        l["Lsmooth"] = gaussian(L, 1.0)
        gx, gy = scharr(l["Lsmooth"], 1, side, centre)
        c = 1.0 / (1.0 + (gx * gx + gy * gy) / (k * k))
        for tau in fed_steps(l["etime"] - p["etime"]):
            L = diffusion_step(L, c, tau, mutation)
        l["Lt"] = L
    for l in levels:
        s = l["sigma_size"]
        norm = 1.0 / (2.0 * s * (10.0 / 3.0 + 2.0))
        deriv = lambda I: tuple(norm * d for d in scharr(I, s, 1.0, 10.0 / 3.0))  # noqa: E731
        l["Lx"], l["Ly"] = deriv(l["Lt"] if mutation == "derivatives_on_lt" else l["Lsmooth"])
        lxx, lxy = deriv(l["Lx"])
        _, lyy = deriv(l["Ly"])
        l["Ldet"] = (lxx * lyy - lxy * lxy) * float(s) ** (2 if mutation == "det_s2" else 4)
    return {"kcontrast": own_k, "k_bin": k_bin, "hmax": hmax, "levels": levels}


# ------------------------------------------------------------------------------------------------ comparing and reporting
def max_errors(got_levels, model_levels):
    """{plane: [max |got - model| per level]} over every pixel"""
    assert len(got_levels) == len(model_levels)
    return {p: [float(np.abs(g[p].astype(np.float64) - m[p]).max()) for g, m in zip(got_levels, model_levels)] for p in PLANES if p in got_levels[0]}


def plane_difference(got, want):
    """None when two float32 planes are equal bit for bit, else what the stage-by-stage probe printed: how many pixels differ, the
    largest difference and the rows / columns that bound them"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape:
        return "shape %s against %s" % (got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if not len(bad):
        return None
    return "%d of %d pixels differ, max |d| %.3g, rows %d..%d, columns %d..%d" % (
        len(bad), got.size, np.nanmax(np.abs(got.astype(np.float64) - want)), bad[:, 0].min(), bad[:, 0].max(), bad[:, 1].min(), bad[:, 1].max())


def bit_parity_report(got_levels, want_levels, planes=("Lt", "Lx", "Ly")):
    """the lines "level i (w x h) plane: ..." of every plane that is not bit-identical, first level first; [] when all are"""
    lines = []
    if len(got_levels) != len(want_levels):
        lines.append("%d levels against %d" % (len(got_levels), len(want_levels)))
    for i, (g, e) in enumerate(zip(got_levels, want_levels)):
        for p in planes:
            d = plane_difference(g[p], e[p])
            if d:
                lines.append("level %d (%d x %d) %s: %s" % (i, e["width"], e["height"], p, d))
    return lines


def tolerance_report(errors, scale=1.0):
    """the entries of `errors` (max_errors) above scale x TOLERANCE as lines naming level, plane, observed and allowed"""
    return ["level %d %s: max |d| %.3g, allowed %.3g" % (i, p, e, scale * TOLERANCE[p][i])
            for p, per_level in errors.items() for i, e in enumerate(per_level) if not e <= scale * TOLERANCE[p][i]]


def measure_oracle_errors(pyoracle):
    """MEASURED, regenerated: the worst oracle-against-model error per (plane, level) over IMAGES"""
    worst = {p: [0.0] * 16 for p in PLANES}
    for name in IMAGES:
        o = pyoracle.akaze_planes(image(name))
        e = max_errors(o["levels"], scale_space(image(name), kcontrast=float(o["kcontrast"]))["levels"])
        for p in PLANES:
            for i, v in enumerate(e[p]):
                worst[p][i] = max(worst[p][i], v)
    return worst


# (measured max |oracle - model| over every pixel and every image of IMAGES, allowed = 4 x measured) per level 0 .. 15; levels
# 12 - 15 exist for the 640 x 320 images only, levels 8 - 11 not for 176 x 96
MEASURED_AND_ALLOWED = {
    "Lt": [
        (2.5e-07, 1.00e-06), (2.7e-07, 1.08e-06), (2.7e-07, 1.08e-06), (2.8e-07, 1.12e-06),    # levels 0 - 3
        (2.4e-07, 9.60e-07), (3.3e-07, 1.32e-06), (2.8e-07, 1.12e-06), (2.9e-07, 1.16e-06),    # levels 4 - 7
        (3.1e-07, 1.24e-06), (3.3e-07, 1.32e-06), (3.1e-07, 1.24e-06), (3.0e-07, 1.20e-06),    # levels 8 - 11
        (6.1e-07, 2.44e-06), (3.1e-07, 1.24e-06), (3.4e-07, 1.36e-06), (8.5e-07, 3.40e-06),    # levels 12 - 15
    ],
    "Lx": [
        (5.4e-08, 2.16e-07), (3.9e-08, 1.56e-07), (4.0e-08, 1.60e-07), (2.8e-08, 1.12e-07),    # levels 0 - 3
        (5.1e-08, 2.04e-07), (4.3e-08, 1.72e-07), (4.3e-08, 1.72e-07), (3.4e-08, 1.36e-07),    # levels 4 - 7
        (5.4e-08, 2.16e-07), (3.4e-08, 1.36e-07), (3.5e-08, 1.40e-07), (2.3e-08, 9.20e-08),    # levels 8 - 11
        (3.5e-08, 1.40e-07), (2.8e-08, 1.12e-07), (3.0e-08, 1.20e-07), (2.0e-08, 8.00e-08),    # levels 12 - 15
    ],
    "Ly": [
        (5.3e-08, 2.12e-07), (3.8e-08, 1.52e-07), (3.9e-08, 1.56e-07), (2.6e-08, 1.04e-07),    # levels 0 - 3
        (4.8e-08, 1.92e-07), (3.7e-08, 1.48e-07), (4.0e-08, 1.60e-07), (2.9e-08, 1.16e-07),    # levels 4 - 7
        (4.5e-08, 1.80e-07), (3.3e-08, 1.32e-07), (3.1e-08, 1.24e-07), (2.4e-08, 9.60e-08),    # levels 8 - 11
        (3.4e-08, 1.36e-07), (2.2e-08, 8.80e-08), (2.8e-08, 1.12e-07), (1.8e-08, 7.20e-08),    # levels 12 - 15
    ],
    "Ldet": [
        (1.2e-08, 4.80e-08), (2.0e-08, 8.00e-08), (2.0e-08, 8.00e-08), (2.4e-08, 9.60e-08),    # levels 0 - 3
        (1.6e-08, 6.40e-08), (3.1e-08, 1.24e-07), (3.2e-08, 1.28e-07), (2.5e-08, 1.00e-07),    # levels 4 - 7
        (1.4e-08, 5.60e-08), (2.0e-08, 8.00e-08), (1.5e-08, 6.00e-08), (1.1e-08, 4.40e-08),    # levels 8 - 11
        (4.7e-09, 1.88e-08), (4.0e-09, 1.60e-08), (4.4e-09, 1.76e-08), (2.1e-09, 8.40e-09),    # levels 12 - 15
    ],
}
MEASURED = {p: [m for m, _ in rows] for p, rows in MEASURED_AND_ALLOWED.items()}
TOLERANCE = {p: [a for _, a in rows] for p, rows in MEASURED_AND_ALLOWED.items()}
# for every level i >= 1 of the EXACT_HALVING images: |mean(Lt[i]) - mean(Lt[0])| of the oracle's planes, the means summed in
# fp64: the largest is 3.0e-9 (level 15 of noisy_640x320), allowed 4 x that
MEASURED_MEAN_DRIFT = 3.0e-9
MEAN_DRIFT_TOLERANCE = 4.0 * MEASURED_MEAN_DRIFT
