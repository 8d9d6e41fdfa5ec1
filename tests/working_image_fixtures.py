"""The working image of the extract stage - what the device computes in front of AKAZE (csrc/akaze.hip, "grey, downscale,
float"; extract_features.cpp:25-27) - as a float64 model written from the definitions, the comparison rule that holds an
8-bit result against it, and the cases.  Plain numpy; no code or table shared with oracle/, csrc/area_table.hpp or
tests/thumbnail_fixtures.py.  `mutation` introduces ONE deliberate error (MUTATIONS) into the model; the CPU test requires
each of them to be seen.

Definitions
  grey     cvtColor(BGR2GRAY), 8 bit: (1868 B + 9617 G + 4899 R + 2^13) >> 14.
  size     cv::resize(fx = fy = scale) with scale = the FLOAT min(1, 1600 / max side) widened to double: W, H = the rint of
           side * scale; nothing is resized when neither side is above 1600.  s = 1 / scale is the footprint of a
           destination pixel in source pixels.
  area     INTER_AREA: destination pixel dx is the mean of the source over its footprint.  The weight of source pixel sx in
           destination dx is the overlap of [dx s, (dx + 1) s) with [sx, sx + 1), sx < ssize, over the footprint's length
           inside the image, min(s, ssize - dx s) (the last cell is shortened, not padded).  Both axes alike: the image is
           multiplied by one overlap matrix per axis.
  slivers  cv's rule, applied as a rule: the overlap with the first or the last source pixel of a footprint is dropped when
           it is at most 1e-3 (a footprint edge that misses a pixel boundary by rounding must not bring in a tap), and the
           remaining weights are NOT renormalised.
  rounding to the nearest 8-bit value, ties to even.  At s = 2 exactly cv::resize takes its integer path, whose vector body -
           the columns below W - W % 16 - computes (a + b + c + d + 2) >> 2: ties go up there.
  float    (float)u8 * (1 / 255f), one float32 product.

The comparison rule (check)
  m = the model's unrounded value in grey levels; tx, ty = the largest number of taps of a footprint per axis.  The device
  sums in float32 with float-rounded weights, one rounding per product and per addition, weights summing to 1 and g <= 255:
  to first order it is off m by at most (tx + ty + 4) 2^-24 255; delta is twice that (1e-4 .. 1e-3 grey levels).  Where
  |frac(m) - 0.5| > delta the 8-bit value must equal round(m); elsewhere (the band) it may differ by one level and no more.
  At s = 2, 4, 8 and where nothing is resized every operation is exact in float32: delta = 0, no band, every pixel - ties
  included - must equal the model's rounding.  The band may hold at most BAND_CAP of a case's pixels: a condition on the
  inputs, asserted on the model alone (on noise at other ratios the share is about 2 delta)."""
import numpy as np

MUTATIONS = (
    "rgb_weights",            # the B and R weights exchanged: RGB input assumed
    "g_r_exchanged",          # the G and R weights exchanged
    "half_up_general",        # ties go up instead of to even on the general path
    "even_in_vector_body",    # ties to even in the vector body at s = 2
    "slivers_kept",           # the sliver rule dropped
    "last_cell_full",         # the last cell divided by s although it ends at the image border
    "box_taps",               # every tap of a footprint weighs 1 / s
)
BAND_CAP = 0.01

# route codes (include/ochip.h: OCHIP_WI_*)
RESIZE_NONE, RESIZE_FUSED4, RESIZE_FUSED8, RESIZE_STAGED_GREY, RESIZE_PER_TAP = range(5)
GREY_FUSED, GREY_GRAY4, GREY_GRAY4_TAIL, GREY_BYTEWISE = range(4)
RESIZE_NAMES = ("none", "fused-4", "fused-8", "staged-from-grey", "per-tap")
GREY_NAMES = ("fused", "gray4", "gray4+tail", "bytewise")


def grey(bgr, mutation=None):
    """cvtColor's fixed-point grey of an (h, w, 3) BGR image, as int64."""
    wb, wg, wr = 1868, 9617, 4899
    if mutation == "rgb_weights":
        wb, wr = wr, wb
    if mutation == "g_r_exchanged":
        wg, wr = wr, wg
    p = bgr.astype(np.int64)
    return (wb * p[:, :, 0] + wg * p[:, :, 1] + wr * p[:, :, 2] + (1 << 13)) >> 14


def working_size(w, h):
    """(W, H, s): the working size and the footprint s = 1 / scale (1.0: nothing is resized)."""
    scale = float(min(np.float32(1.0), np.float32(1600.0) / np.float32(max(w, h))))
    W, H = int(np.rint(w * scale)), int(np.rint(h * scale))
    return W, H, 1.0 / scale


def overlap_band(ssize, dsize, s, mutation=None):
    """The overlap matrix of one axis (dsize x ssize) stored by its band: row dx holds the source pixels first[dx] + k,
    k < K, with weight[dx, k] (0 where the footprint does not reach).  Returns (first, weight, taps per row)."""
    K = int(np.ceil(s)) + 2
    dx = np.arange(dsize, dtype=np.float64)[:, None]
    lo, hi = dx * s, (dx + 1.0) * s
    first = np.floor(lo).astype(np.int64)
    sx = first + np.arange(K)[None, :]
    ov = np.minimum(np.minimum(hi, sx + 1.0), float(ssize)) - np.maximum(lo, sx.astype(np.float64))
    ov = np.where(sx < ssize, np.maximum(ov, 0.0), 0.0)
    if mutation != "slivers_kept":
        rows = np.arange(dsize)
        nz = ov > 0.0
        head = np.argmax(nz, axis=1)                            # first and last pixel the footprint touches
        tail = K - 1 - np.argmax(nz[:, ::-1], axis=1)
        for at in (head, tail):
            sliver = ov[rows, at] <= 1e-3
            ov[rows[sliver], at[sliver]] = 0.0
    cell = np.minimum(s, ssize - lo)
    if mutation == "last_cell_full":
        cell = np.full_like(lo, s)
    if mutation == "box_taps":
        ov = np.where(ov > 0.0, 1.0, 0.0)
        cell = np.full_like(lo, s)
    weight = ov / cell
    return first[:, 0], weight, np.count_nonzero(weight, axis=1)


def apply_band(img, first, weight, ssize):
    """img (rows x ssize) times the transposed overlap matrix of the band: rows x dsize."""
    out = np.zeros((img.shape[0], len(first)))
    for k in range(weight.shape[1]):
        out += img[:, np.minimum(first + k, ssize - 1)] * weight[None, :, k]     # (a clamped index meets a zero weight)
    return out


class Shape:
    """What depends on the source size alone: the working size, s, the overlap bands and the largest tap counts."""

    def __init__(self, w, h, mutation=None):
        assert mutation is None or mutation in MUTATIONS, mutation
        self.w, self.h = w, h
        self.W, self.H, self.s = working_size(w, h)
        self.resized = (self.W, self.H) != (w, h)
        self.xband = self.yband = None
        self.tx = self.ty = 1
        if self.resized:
            self.xband = overlap_band(w, self.W, self.s, mutation)
            self.yband = overlap_band(h, self.H, self.s, mutation)
            self.tx, self.ty = int(self.xband[2].max()), int(self.yband[2].max())
        self.exact = not self.resized or self.s in (2.0, 4.0, 8.0)
        self.delta = 0.0 if self.exact else 2.0 * (self.tx + self.ty + 4) * 2.0 ** -24 * 255.0


class Model(Shape):
    """The model of one image: m (H x W float64, unrounded grey levels), u8 (its rounding by the rules above), delta and
    band (the pixels whose rounding float32 may decide either way)."""

    def __init__(self, bgr, mutation=None):
        h, w, _ = bgr.shape
        Shape.__init__(self, w, h, mutation)
        g = grey(bgr, mutation).astype(np.float64)
        if not self.resized:
            self.m = g
        else:
            rows = apply_band(g, self.xband[0], self.xband[1], w)                           # h x W
            self.m = apply_band(rows.T, self.yband[0], self.yband[1], h).T                  # H x W
        frac = self.m - np.floor(self.m)
        self.band = np.abs(frac - 0.5) <= self.delta if self.delta > 0.0 else np.zeros(self.m.shape, bool)
        even = np.rint(self.m)
        up = np.floor(self.m + 0.5)
        r = up if mutation == "half_up_general" else even
        if self.resized and self.s == 2.0:
            body = self.W - self.W % 16
            r[:, :body] = (even if mutation == "even_in_vector_body" else up)[:, :body]
        self.u8 = np.clip(r, 0, 255).astype(np.uint8)

    @property
    def band_share(self):
        return float(self.band.mean())


def check(got_u8, model):
    """The comparison rule.  Returns the figures: band share, pixels outside the band that differ from the model's rounding,
    the largest difference in levels anywhere, and the worst |got - m| outside the band.  passed(figures) says whether
    they meet the rule."""
    assert got_u8.shape == model.m.shape and got_u8.dtype == np.uint8, (got_u8.shape, model.m.shape, got_u8.dtype)
    diff = got_u8.astype(np.int64) - model.u8.astype(np.int64)
    out = ~model.band
    return {
        "band_share": model.band_share,
        "wrong_outside": int(np.count_nonzero(diff[out])),
        "worst_levels": int(np.abs(diff).max()),
        "worst_outside": float(np.abs(got_u8[out] - model.m[out]).max()) if out.any() else 0.0,
        "pixels": int(diff.size),
    }


def passed(f):
    return f["wrong_outside"] == 0 and f["worst_levels"] <= 1 and f["band_share"] <= BAND_CAP


def mutation_seen(f):
    """How a mutated model has to fail against a correct image: a difference above one level, or more than BAND_CAP of
    the pixels differing outside the band."""
    return f["worst_levels"] > 1 or f["wrong_outside"] > BAND_CAP * f["pixels"]


def floats_of(u8):
    """(float)u8 * (1 / 255f) in float32."""
    return u8.astype(np.float32) * (np.float32(1.0) / np.float32(255.0))


def u8_of(floats):
    """The 8-bit image behind the device's floats, or an AssertionError when they are not floats_of(an 8-bit image) to
    the bit."""
    u8 = np.clip(np.rint(floats.astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
    assert np.array_equal(floats_of(u8).view(np.uint32), floats.view(np.uint32)), "not (float)u8 * (1 / 255f)"
    return u8


# ---- the dispatch of csrc/akaze.hip restated over the model's taps
RS_PITCH, RS_ROWS, RESIZE_ROWS, RESIZE_MAX_TAPS, BLOCK_COLS = 704, 32, 8, 8, 256


def routes(model, aligned=True, n_images=1):
    """(resize route, grey route) the device has to report for a Shape or Model: a source whose width is a multiple of 4
    is staged in LDS when every block of 256 destination columns reads at most 701 source columns from its first one
    rounded down to a multiple of 4, no column has more than 8 taps, and every 8 destination rows read at most 32 source
    rows; a 4-byte aligned source is then converted to grey on the way in (fused), unrolled to 4 taps when no column has
    more; an unstaged or unaligned source is converted first: four pixels a thread when aligned (the last n_px % 4 byte
    by byte), byte by byte otherwise."""
    n_px = model.w * model.h * n_images
    staged = False
    most = 0
    if model.resized:
        xf, xw, xn = model.xband
        yf, yw, yn = model.yband
        xs0 = xf + np.argmax(xw > 0, axis=1)                  # first and last tap of every column / row
        xs1 = xs0 + xn - 1
        ys0 = yf + np.argmax(yw > 0, axis=1)
        ys1 = ys0 + yn - 1
        most = int(xn.max())
        staged = model.w % 4 == 0 and most <= RESIZE_MAX_TAPS
        for x0 in range(0, model.W, BLOCK_COLS):
            x1 = min(x0 + BLOCK_COLS, model.W)
            staged = staged and int(xs1[x1 - 1]) - (int(xs0[x0]) & ~3) + 1 <= RS_PITCH - 3
        for y0 in range(0, model.H, RESIZE_ROWS):
            y1 = min(y0 + RESIZE_ROWS, model.H)
            staged = staged and int(ys1[y1 - 1]) - int(ys0[y0]) + 1 <= RS_ROWS
    fused = staged and aligned
    if not model.resized:
        resize = RESIZE_NONE
    elif fused:
        resize = RESIZE_FUSED4 if most <= 4 else RESIZE_FUSED8
    else:
        resize = RESIZE_STAGED_GREY if staged else RESIZE_PER_TAP
    if fused:
        g = GREY_FUSED
    elif aligned:
        g = GREY_GRAY4_TAIL if n_px % 4 else GREY_GRAY4
    else:
        g = GREY_BYTEWISE
    return resize, g


# ---- images
def noise(w, h, seed):
    """Uniform colour noise, B, G and R independent: a wrong weight or byte lane moves about a third of all pixels."""
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def primaries(w, h):
    """Saturated primaries in stripes one pixel wide, narrower than any footprint: pure B, G, R, white, black, the phase
    moving by two from row to row; a level of noise in the lowest bits keeps footprint means off exact ties."""
    colours = np.array([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 255), (0, 0, 0)], np.int64)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    img = colours[(x + 2 * y) % 5]
    dirt = np.random.default_rng(w * 7 + h).integers(0, 8, (h, w, 3))
    return np.where(img > 0, img - dirt, img + dirt).astype(np.uint8)


def tinted_blobs(w, h, seed):
    """The suite's blob scenes with a colour tint (tests/test_gpu_extract.py: test_grey_and_area_resize)."""
    from opencalibration_amd import synth

    rng = np.random.default_rng(seed)
    base = synth.render_blobs(w, h, seed)
    tint = rng.integers(0, 40, (h, w, 3), dtype=np.uint8)
    return np.clip(base.astype(np.int32) + tint - 20, 0, 255).astype(np.uint8)


def image(kind, w, h, seed):
    if kind == "noise":
        return noise(w, h, seed)
    if kind == "primaries":
        return primaries(w, h)
    if kind == "sliver":        # noise under a white second row: the sliver a footprint of the first row would take from it is worth most
        img = noise(w, h, seed)
        img[1] = 255
        return img
    assert kind == "blobs", kind
    return tinted_blobs(w, h, seed)


# ---- cases: (name, width, height, image kind, expected resize route for an aligned source, why)
# The smallest shapes that reach their route.  `offsets`: the byte offsets of the device buffer the GPU test also runs.
class Case:
    def __init__(self, name, w, h, kind, resize, grey_route, why, offsets=(), seed=None):
        self.name, self.w, self.h, self.kind, self.resize, self.grey, self.why, self.offsets = name, w, h, kind, resize, grey_route, why, offsets
        self.seed = seed if seed is not None else w * 31 + h

    def image(self):
        return image(self.kind, self.w, self.h, self.seed)

    def __repr__(self):
        return self.name


CASES = (
    Case("4000x100", 4000, 100, "noise", RESIZE_FUSED4, GREY_FUSED, "the headline 2.5 : 1, 3 taps, a partial last block", offsets=(1, 2, 3)),
    Case("4000x100-primaries", 4000, 100, "primaries", RESIZE_FUSED4, GREY_FUSED, "saturated primaries through the dot-product grey", offsets=(1,)),
    Case("4000x100-blobs", 4000, 100, "blobs", RESIZE_FUSED4, GREY_FUSED, "the suite's blobs, tinted"),
    Case("4376x100", 4376, 100, "noise", RESIZE_FUSED4, GREY_FUSED, "4 taps, the widest source whose window still fits the tile"),
    Case("4380x100", 4380, 100, "noise", RESIZE_PER_TAP, GREY_GRAY4, "4 taps, the window no longer fits"),
    Case("1604x100", 1604, 100, "noise", RESIZE_FUSED4, GREY_FUSED, "s = 1.0025: footprints that end on pixel borders up to rounding, a short last row"),
    Case("1601x3", 1601, 3, "sliver", RESIZE_PER_TAP, GREY_GRAY4_TAIL, "s = 1.000625: the first of three rows ends 0.000625 inside the second, a white one; n_px % 4 = 3"),
    Case("3200x96", 3200, 96, "noise", RESIZE_FUSED4, GREY_FUSED, "exact 2, every column in the vector body"),
    Case("40x3200", 40, 3200, "noise", RESIZE_FUSED4, GREY_FUSED, "exact 2, 16 columns of vector body and 4 of scalar tail, W < 256"),
    Case("400x5004", 400, 5004, "noise", RESIZE_FUSED8, GREY_FUSED, "5 horizontal taps while staged: tall and narrow"),
    Case("2002x100", 2002, 100, "noise", RESIZE_PER_TAP, GREY_GRAY4, "a width that is no multiple of 4"),
    Case("2002x100-primaries", 2002, 100, "primaries", RESIZE_PER_TAP, GREY_GRAY4, "saturated primaries through every byte lane of gray4"),
    Case("6400x64", 6400, 64, "noise", RESIZE_PER_TAP, GREY_GRAY4, "exact 4: compared everywhere, ties included"),
    Case("12000x100", 12000, 100, "noise", RESIZE_PER_TAP, GREY_GRAY4, "8 horizontal taps, still unrolled"),
    Case("16000x100", 16000, 100, "noise", RESIZE_PER_TAP, GREY_GRAY4, "10 and more horizontal taps, taken from the table"),
    Case("33x21", 33, 21, "noise", RESIZE_NONE, GREY_GRAY4_TAIL, "not resized, n_px % 4 = 1", offsets=(1, 2, 3)),
    Case("33x21-primaries", 33, 21, "primaries", RESIZE_NONE, GREY_GRAY4_TAIL, "not resized, saturated primaries", offsets=(3,)),
    Case("64x64", 64, 64, "noise", RESIZE_NONE, GREY_GRAY4, "not resized, whole dwords", offsets=(1, 2, 3)),
)
CASE = {c.name: c for c in CASES}
_BUILT = {}


def built(name):
    """(image, model) of a case, built once per process and read-only."""
    if name not in _BUILT:
        img = CASE[name].image()
        model = Model(img)
        for a in (img, model.m, model.u8, model.band):
            a.setflags(write=False)
        _BUILT[name] = (img, model)
    return _BUILT[name]

# the batch of the GPU test: three different images of the headline shape in one call (the kernels' blockIdx.z offsets)
BATCH = ("4000x100", "4000x100-primaries", "4000x100-blobs")

# where each mutation has to be seen
MUTATION_CASES = {
    "rgb_weights": ("4000x100", "33x21"),
    "g_r_exchanged": ("4000x100", "2002x100-primaries"),
    "half_up_general": ("6400x64", "40x3200"),
    "even_in_vector_body": ("3200x96", "40x3200"),
    "slivers_kept": ("1601x3",),
    "last_cell_full": ("1604x100",),
    "box_taps": ("4000x100", "12000x100"),
}
